// g2048_device.h -- per-lane 2048 board arithmetic for gfx950 (CDNA4), one board per lane.
//
// A board is 16 cells of int8 exponents (0 = empty, k = tile 2^k), row-major, held in four
// 32-bit VGPRs r[0..3] (r[i] byte j = cell (i, j)).  Every exponent is < 0x80 (really <= 17),
// which makes the classic "SIMD within a register" byte tricks carry-free.
//
// Reference semantics (cited as game2048_env.py:LINE = /root/reference/env/envs/game2048_env.py):
//   move   :194-241   four lines, each through shift(); direction 0 up, 1 right, 2 down, 3 left
//   shift  :243-260   compact non-zeros, merge equal neighbours once, leftmost first
//   add_tile :166-176 value then position (uniform over the empty cells)
//   isend  :262-280   max_tile reached, else any empty -> False, else no legal move
//   highest :190-192
//
// The slide/merge runs on all four lines at once: the board is re-expressed as four registers
// A,B,C,D where byte l of A is the FIRST cell of line l (in shift order), B the second, ... so
// one 32-bit VALU op advances four lines.  For vertical moves A..D are simply the rows (reversed
// for "down"); for horizontal moves they are the columns.  Two formulations of that re-expression:
// move() -- an 8 x v_perm_b32 byte transpose plus lane-mask selects -- and move_sel(), the one the
// step kernels use: a two-stage v_perm network whose byte selectors come from a 4-row table, so the
// direction costs no select instructions at all.  No cross-lane traffic: the step lives in ~42 VGPRs.
#pragma once

#include <stdint.h>

#if defined(G2048_HOST_CHECK)
// Host compilation of this header exists ONLY for tests/host_check (a g++-built unit test of the
// SWAR math against the oracle in this GPU-less container).  The product never runs this path.
#define G2048_DEV static inline
static inline uint32_t g2048_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int k = 0; k < 4; ++k) {
        uint32_t s = (sel >> (8 * k)) & 0xff;
        uint32_t byte = s < 8 ? (uint32_t)((src >> (8 * s)) & 0xff) : (s == 12 ? 0u : 0xffu);
        out |= byte << (8 * k);
    }
    return out;
}
static inline uint32_t g2048_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
static inline uint32_t g2048_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
static inline uint32_t g2048_clz(uint32_t x) { return (uint32_t)__builtin_clz(x); }   // x != 0
static inline uint32_t g2048_funnel_shr(uint32_t hi, uint32_t lo, uint32_t k) // low word of (hi:lo) >> k, 0 <= k <= 31
{
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (k & 31u));
}
static inline uint32_t g2048_ctz(uint32_t x) { return (uint32_t)__builtin_ctz(x); }   // x != 0
static inline float g2048_rcp(float x) { return 1.0f / x; }
static inline uint32_t g2048_opaque(uint32_t x) { return x; }
static inline uint32_t g2048_bfi(uint32_t m, uint32_t a, uint32_t b) { return (m & a) | (~m & b); }
static inline bool g2048_any(bool x) { return x; }
static inline uint32_t g2048_xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
template <int K> static inline uint32_t g2048_pow2_byte(uint32_t x, uint32_t) { return 1u << ((x >> (8 * K)) & 31u); }
#else
#include <hip/hip_runtime.h>
#define G2048_DEV __device__ __forceinline__
G2048_DEV uint32_t g2048_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
G2048_DEV uint32_t g2048_mulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
G2048_DEV uint32_t g2048_popc(uint32_t x) { return (uint32_t)__popc(x); }
G2048_DEV uint32_t g2048_clz(uint32_t x) { return (uint32_t)__builtin_clz(x); }   // x != 0: v_ffbh_u32
// low word of (hi:lo) >> k, 0 <= k <= 31: v_alignbit_b32
G2048_DEV uint32_t g2048_funnel_shr(uint32_t hi, uint32_t lo, uint32_t k) { return __builtin_amdgcn_alignbit(hi, lo, k); }
G2048_DEV uint32_t g2048_ctz(uint32_t x) { return (uint32_t)__builtin_ctz(x); }   // x != 0: v_ffbl_b32
G2048_DEV float g2048_rcp(float x) { return __builtin_amdgcn_rcpf(x); }               // x normal: v_rcp_f32, 1 ulp
// Hides a value's origin from the optimizer.  Used on lane-wide select masks: without it LLVM turns
// "(m & a) | (~m & b)" with m = -(cond) back into v_cndmask_b32_e64 (4 issue cycles) instead of one
// v_bitop3_b32 (2 cycles).
G2048_DEV uint32_t g2048_opaque(uint32_t x)
{
    asm volatile("" : "+v"(x));
    return x;
}
// (m & a) | (~m & b) as ONE v_bitop3_b32 (2 issue cycles; v_bfi_b32 / v_cndmask_e64 take 4).
G2048_DEV uint32_t g2048_bfi(uint32_t m, uint32_t a, uint32_t b) { return __builtin_amdgcn_bitop3_b32(m, a, b, 0xCA); }
// a ^ b ^ c as ONE v_bitop3_b32 (the compiler emits two v_xor_b32 for the Philox rounds otherwise).
G2048_DEV uint32_t g2048_xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
// 1 << (byte K of x, low five bits) as ONE instruction: SDWA selects the byte as the shift operand of
// v_lshlrev_b32 (the compiler emits a v_lshrrev + v_lshl_add pair per byte otherwise).  `one` = a VGPR holding 1.
template <int K> G2048_DEV uint32_t g2048_pow2_byte(uint32_t x, uint32_t one)
{
    uint32_t r;
    if constexpr (K == 0)
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(r) : "v"(x), "v"(one));
    else if constexpr (K == 1)
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(r) : "v"(x), "v"(one));
    else if constexpr (K == 2)
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(r) : "v"(x), "v"(one));
    else
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(r) : "v"(x), "v"(one));
    return r;
}
// true when the predicate holds in any active lane of the wavefront (wave-uniform).  The builtin takes the
// predicate as a lane mask; HIP's __ballot(int) would first materialise it as 0/1 in a VGPR and compare again.
G2048_DEV bool g2048_any(bool x) { return __builtin_amdgcn_ballot_w64(x) != 0ull; }
#endif

namespace g2048 {

struct Board {
    uint32_t r[4];
};

// Board i of an array of 16-byte boards: one global_load_dwordx4 per lane
#if defined(G2048_HOST_CHECK)
struct uint4 {
    uint32_t x, y, z, w;
};
G2048_DEV Board load_board(const uint4 *boards, uint32_t i)
{
    Board b;
    __builtin_memcpy(b.r, boards + i, 16); // the tests' arrays are bytes
    return b;
}
#else
G2048_DEV Board load_board(const uint4 *boards, uint32_t i)
{
    const uint4 v = boards[i];
    return Board{{v.x, v.y, v.z, v.w}};
}
#endif

// ------------------------------------------------------------------------------------ Philox
// Philox4x32-10, constants as in rocrand_philox4x32_10.h:62-65.  The spawn stream:
//   word(seed, t, board, slot) = Philox(ctr = (t_lo, t_hi, board, slot >> 2), key = seed)[slot & 3]
// Every batched path needs slots 0..2 (+ word 3 for the synthetic random policy), i.e. ONE block
// per board per step and no per-board RNG state in HBM.
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct Words {
    uint32_t w[4];
};

G2048_DEV Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0;
        const uint64_t p1 = (uint64_t)kPhiloxM1 * c2;
        // At every call site c0, c1, c3 and the key are wave-uniform (t, slot, seed) and only c2 (the board) is
        // per lane.  Rounds 0..2 therefore pair the two uniform terms of each xor3 with plain xors, so they --
        // and round 1's whole M1 * c2 product -- stay on the scalar unit (one v_xor with an SGPR operand per
        // word); the bitop3 builtin is VALU-only and would cost a v_mov per second SGPR operand.
        uint32_t n0, n2;
        if (round == 0) {
            n0 = (uint32_t)(p1 >> 32) ^ (c1 ^ k0);
            n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        } else if (round == 1) {
            n0 = c1 ^ ((uint32_t)(p1 >> 32) ^ k0);
            n2 = (uint32_t)(p0 >> 32) ^ (c3 ^ k1);
        } else if (round == 2) {
            n0 = (uint32_t)(p1 >> 32) ^ (c1 ^ k0);            // c1 = low word of round 1's uniform product
            n2 = g2048_xor3((uint32_t)(p0 >> 32), c3, k1);
        } else {
            n0 = g2048_xor3((uint32_t)(p1 >> 32), c1, k0);
            n2 = g2048_xor3((uint32_t)(p0 >> 32), c3, k1);
        }
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return Words{{c0, c1, c2, c3}};
}

// ------------------------------------------------------------------------- SWAR byte helpers
// All inputs have every byte < 0x80.
constexpr uint32_t kLow7 = 0x7f7f7f7fu, kHigh1 = 0x80808080u;

// 0x80 in every non-zero byte.
G2048_DEV uint32_t nz80(uint32_t x) { return (x + kLow7) & kHigh1; }
// 0x80 in every zero byte.
G2048_DEV uint32_t z80(uint32_t x) { return ~(x + kLow7) & kHigh1; }
// 0x80 flags -> 0x7f byte masks (enough to select bytes < 0x80).
G2048_DEV uint32_t mask7(uint32_t f80) { return f80 - (f80 >> 7); }
// (m & a) | (~m & b)
G2048_DEV uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) { return g2048_bfi(m, a, b); }

// 4x4 byte transpose: rows -> columns (and back; it is an involution).
G2048_DEV Board transpose(const Board &b)
{
    const uint32_t x0 = g2048_perm(b.r[1], b.r[0], 0x05010400u);
    const uint32_t x1 = g2048_perm(b.r[1], b.r[0], 0x07030602u);
    const uint32_t x2 = g2048_perm(b.r[3], b.r[2], 0x05010400u);
    const uint32_t x3 = g2048_perm(b.r[3], b.r[2], 0x07030602u);
    Board t;
    t.r[0] = g2048_perm(x2, x0, 0x05040100u);
    t.r[1] = g2048_perm(x2, x0, 0x07060302u);
    t.r[2] = g2048_perm(x3, x1, 0x05040100u);
    t.r[3] = g2048_perm(x3, x1, 0x07060302u);
    return t;
}

// 0x7f in every non-zero byte (a byte-select mask; all data bytes are < 0x80).
G2048_DEV uint32_t nzmask(uint32_t x) { return mask7(nz80(x)); }
// all-ones when cond, else 0 (lane-wide select mask; selects then cost one v_bitop3 each).
G2048_DEV uint32_t lanemask(bool cond) { return g2048_opaque(0u - (cond ? 1u : 0u)); }
// the same from bit 0 of an integer, without a compare
G2048_DEV uint32_t lanemask_bit0(uint32_t x) { return g2048_opaque(0u - (x & 1u)); }

// game2048_env.py:243-260 for four lines at once.  a,b,c,d: 1st..4th cell of each line.
// Returns the summed merge score of the four lines.
//
// Issue-cost notes (measured on gfx950, tools/ubench/valu_ubench.hip): VOP2 integer ops and
// v_bitop3_b32 issue in 2 cycles, v_perm / v_bcnt / v_cndmask_e64 / multiplies in 4.  Everything
// below is therefore phrased as three-input boolean functions of byte masks.
G2048_DEV uint32_t shift4(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d)
{
    // -- compaction by rank (game2048_env.py:249-251 skips zeros): the j-th output is the j-th
    //    non-zero cell.  ka/kb/kc = "cell is non-zero" byte masks.
    const uint32_t ka = nzmask(a), kb = nzmask(b), kc = nzmask(c);
    const uint32_t one_ab = ka ^ kb;                                  // exactly one of a,b
    const uint32_t all_abc = ka & kb & kc;
    const uint32_t one_abc = (ka ^ kb ^ kc) & ~all_abc;               // exactly one of a,b,c
    const uint32_t two_abc = ((ka & kb) | (kc & (ka | kb))) & ~all_abc; // exactly two of a,b,c
    const uint32_t p0 = bfi(ka, a, bfi(kb, b, bfi(kc, c, d)));        // first non-zero
    const uint32_t p1 = (b & ka) | (c & one_ab) | (d & one_abc);      // second
    const uint32_t p2 = (c & ka & kb) | (d & two_abc);                // third
    const uint32_t p3 = d & all_abc;                                  // fourth
    // -- merge flags (0x80 per byte): a pair merges when equal and non-zero; leftmost first, each
    //    cell once (:252-255).  After compaction p[j+1] != 0 implies p[j] != 0.
    const uint32_t s1 = p1 + kLow7, s2 = p2 + kLow7, s3 = p3 + kLow7; // bit 7 = non-zero
    const uint32_t eab = ~((p0 ^ p1) + kLow7) & s1 & kHigh1;
    const uint32_t ebc = ~((p1 ^ p2) + kLow7) & s2 & kHigh1 & ~eab;
    const uint32_t ecd = ~((p2 ^ p3) + kLow7) & s3 & kHigh1 & ~ebc;
    const uint32_t iab = eab >> 7, ibc = ebc >> 7, icd = ecd >> 7;    // +1 on the exponent
    const uint32_t mab = eab - iab, mbc = ebc - ibc, mcd = ecd - icd; // 0x7f masks
    const uint32_t a1 = p0 + iab, b1 = p1 + ibc, c1 = p2 + icd;
    // -- outputs
    a = a1;
    b = bfi(mab, c1, b1);
    c = bfi(mab, p3 & ~mcd, bfi(mbc, p3, c1));
    d = p3 & ~(mab | mbc | mcd);
    // -- score: sum of 2^e over the merged cells (:253-254).  v_lshlrev uses only the low five bits
    //    of the shift operand, so "1 << (x >> 8l)" needs no byte extraction; bytes without a merge
    //    are set to 31, whose 2^31 terms can only disturb bit 31, which the final mask drops.
    const uint32_t m1 = bfi(mab, a1, bfi(mbc, b1, 0x1f1f1f1fu)); // first merge of each line
    const uint32_t m2 = bfi(mcd, c1, 0x1f1f1f1fu);               // second merge of each line
    const uint32_t one = g2048_opaque(1u);
    const uint32_t score = (g2048_pow2_byte<0>(m1, one) + g2048_pow2_byte<1>(m1, one) + g2048_pow2_byte<2>(m1, one)) +
                           (g2048_pow2_byte<3>(m1, one) + g2048_pow2_byte<0>(m2, one) + g2048_pow2_byte<1>(m2, one)) +
                           (g2048_pow2_byte<2>(m2, one) + g2048_pow2_byte<3>(m2, one));
    return score & 0x7fffffffu;
}

// game2048_env.py:194-241.  Returns true when the board changed (false = IllegalMove).
G2048_DEV bool move(Board &bd, uint32_t action, uint32_t &score)
{
    const uint32_t hz = lanemask_bit0(action);                 // :211 dir_mod_two
    const uint32_t rv = lanemask_bit0(action ^ (action >> 1)); // :212 shift_direction
    const Board t = transpose(bd);
    const uint32_t l0 = bfi(hz, t.r[0], bd.r[0]), l1 = bfi(hz, t.r[1], bd.r[1]);
    const uint32_t l2 = bfi(hz, t.r[2], bd.r[2]), l3 = bfi(hz, t.r[3], bd.r[3]);
    uint32_t a = bfi(rv, l3, l0), b = bfi(rv, l2, l1), c = bfi(rv, l1, l2), d = bfi(rv, l0, l3);
    const uint32_t a0 = a, b0 = b, c0 = c, d0 = d;
    score = shift4(a, b, c, d);
    const bool changed = ((a ^ a0) | (b ^ b0) | (c ^ c0) | (d ^ d0)) != 0; // :222,234,238
    Board o;
    o.r[0] = bfi(rv, d, a);
    o.r[1] = bfi(rv, c, b);
    o.r[2] = bfi(rv, b, c);
    o.r[3] = bfi(rv, a, d);
    const Board ot = transpose(o);
    bd.r[0] = bfi(hz, ot.r[0], o.r[0]);
    bd.r[1] = bfi(hz, ot.r[1], o.r[1]);
    bd.r[2] = bfi(hz, ot.r[2], o.r[2]);
    bd.r[3] = bfi(hz, ot.r[3], o.r[3]);
    return changed;
}

// Number of empty cells.
G2048_DEV uint32_t count_empty(const Board &bd)
{
    return g2048_popc(z80(bd.r[0]) | (z80(bd.r[1]) >> 1) | (z80(bd.r[2]) >> 2) | (z80(bd.r[3]) >> 3));
}

// The spawn word w on a board with n empty cells (game2048_env.py:166-176), read off the 64-bit product p = w * n:
//   position  k = p >> 32: the k-th empty cell in row-major order (= floor(u * n), u = w / 2^32);
//   value     2 (exponent 1) if (uint32_t)p <= kTwoThreshold else 4, i.e. frac(u * n) < 0.9 (:168) -- the part of the
//             word the position did not use: uniform and independent of k up to the word's resolution, so P(2) is
//             within n / 2^32 < 4e-9 of the reference's 0.9.
constexpr uint32_t kTwoThreshold = 3865470566u; // r / 2^32 < 0.9  <=>  r <= 3865470566

// `enable` (all-ones / 0) gates the write.  Returns the number of empty cells BEFORE the spawn; `is2` = "the new
// tile is a 2" (the callers that keep the score deficit need it as well).
G2048_DEV uint32_t add_tile(Board &bd, uint32_t w, uint32_t enable, bool &is2)
{
    const uint32_t z0 = z80(bd.r[0]), z1 = z80(bd.r[1]), z2 = z80(bd.r[2]), z3 = z80(bd.r[3]);
    const uint32_t c0 = g2048_popc(z0), c1 = c0 + g2048_popc(z1), c2 = c1 + g2048_popc(z2),
                   n = c2 + g2048_popc(z3);
    const uint64_t p = static_cast<uint64_t>(w) * n;
    const uint32_t k = static_cast<uint32_t>(p >> 32);
    is2 = static_cast<uint32_t>(p) <= kTwoThreshold;
    // row of the k-th empty cell: g_i = all-ones when k >= c_i (nested: g2 implies g1 implies g0)
    const uint32_t g0 = (uint32_t)((int32_t)(c0 - 1u - k) >> 31), g1 = (uint32_t)((int32_t)(c1 - 1u - k) >> 31),
                   g2 = (uint32_t)((int32_t)(c2 - 1u - k) >> 31);
    const uint32_t zs = bfi(g2, z3, bfi(g1, z2, bfi(g0, z1, z0)));     // empty flags of that row
    const uint32_t base = bfi(g2, c2, bfi(g1, c1, c0 & g0));           // empties before that row
    // inside the row: inclusive prefix count of the empty flags per byte; the target byte is the
    // empty one whose count equals kk + 1
    const uint32_t want = (k - base + 1u) * 0x01010101u;
    const uint32_t prefix = (zs >> 7) * 0x01010101u;
    const uint32_t hit = ~((prefix ^ want) + kLow7) & zs;              // 0x80 at the chosen cell only
    // exponent 1 -> 0x01 at that byte (hit >> 7), exponent 2 -> 0x02 (hit >> 6)
    const uint32_t tile = (hit >> (is2 ? 7u : 6u)) & enable;
    // one-hot row masks from the nested g's (kept as values: one v_bitop3 per row instead of compare + select)
    const uint32_t h0 = g2048_opaque(g0), h1 = g2048_opaque(g1), h2 = g2048_opaque(g2);
    bd.r[0] |= tile & ~h0;
    bd.r[1] |= tile & (h0 ^ h1);
    bd.r[2] |= tile & (h1 ^ h2);
    bd.r[3] |= tile & h2;
    return n;
}

G2048_DEV uint32_t add_tile(Board &bd, uint32_t w, uint32_t enable = 0xffffffffu)
{
    bool is2;
    return add_tile(bd, w, enable, is2);
}

// The two spawns of a reset (game2048_env.py:108-109) on the empty board: the first word meets 16 empty cells
// (k = w1 >> 28, fraction = w1 << 4), the second 15.
G2048_DEV bool fresh_is_four_16(uint32_t w1) { return (w1 << 4) > kTwoThreshold; }
G2048_DEV bool fresh_is_four_15(uint32_t w2) { return w2 * 15u > kTwoThreshold; }

// game2048_env.py:102-111: empty board + two spawns from words w1, w2.
G2048_DEV Board fresh_board(uint32_t w1, uint32_t w2)
{
    const uint32_t p1 = w1 >> 28;                  // (w1 * 16) >> 32: cell of the first tile
    const uint32_t k2 = g2048_mulhi(w2, 15u);
    const uint32_t p2 = k2 + (k2 >= p1 ? 1u : 0u); // k2-th empty cell, skipping p1
    const uint32_t e1 = fresh_is_four_16(w1) ? 2u : 1u;
    const uint32_t e2 = fresh_is_four_15(w2) ? 2u : 1u;
    // place each exponent in a 64-bit half (cells 0-7 / 8-15) with one 64-bit shift
    const uint64_t x1 = (uint64_t)e1 << (8u * (p1 & 7u)), x2 = (uint64_t)e2 << (8u * (p2 & 7u));
    const uint32_t h1 = lanemask_bit0(p1 >> 3), h2 = lanemask_bit0(p2 >> 3); // upper half?
    const uint32_t x1l = (uint32_t)x1, x1h = (uint32_t)(x1 >> 32), x2l = (uint32_t)x2, x2h = (uint32_t)(x2 >> 32);
    Board bd;
    bd.r[0] = (x1l & ~h1) | (x2l & ~h2);
    bd.r[1] = (x1h & ~h1) | (x2h & ~h2);
    bd.r[2] = (x1l & h1) | (x2l & h2);
    bd.r[3] = (x1h & h1) | (x2h & h2);
    return bd;
}

// True when two neighbouring cells (horizontally or vertically) are equal.  Only meaningful on a
// FULL board, where it is exactly "some move is legal" (game2048_env.py:273-279).
G2048_DEV bool has_equal_neighbours(const Board &bd)
{
    uint32_t f = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        f |= z80(bd.r[i] ^ (bd.r[i] >> 8)) & 0x00808080u;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        f |= z80(bd.r[i] ^ bd.r[i + 1]);
    return f != 0;
}

// Bytewise max of two SWAR words.
G2048_DEV uint32_t max4(uint32_t x, uint32_t y)
{
    const uint32_t ge = mask7(((x | kHigh1) - y) & kHigh1); // 0x7f where x >= y
    return bfi(ge, x, y);
}

// game2048_env.py:190-192 as an exponent.
G2048_DEV uint32_t highest(const Board &bd)
{
    uint32_t m = max4(max4(bd.r[0], bd.r[1]), max4(bd.r[2], bd.r[3]));
    m = max4(m, m >> 16);
    m = max4(m, m >> 8);
    return m & 0xffu;
}

// game2048_env.py:262-280.  max_exp: log2(max_tile), 0 = None.
G2048_DEV bool is_end(const Board &bd, uint32_t max_exp)
{
    bool end = false;
    if (count_empty(bd) == 0)                             // :270-271
        end = !has_equal_neighbours(bd);                  // :273-280
    if (max_exp != 0 && highest(bd) == max_exp)           // :267-268
        end = true;
    return end;
}

// ------------------------------------------------------------ direction by per-lane selectors
// The same move() without the select network: v_perm_b32 takes its byte selector from a VGPR, so
// a two-stage perm network whose SELECTORS depend on the lane's action maps the board straight to
// the shift-order registers A..D (reversal included) and back -- 16 v_perm, no v_bitop3 selects.
//   stage 1: x0 = perm(r1, r0, sa)  x1 = perm(r1, r0, sb)  x2 = perm(r3, r2, sa)  x3 = perm(r3, r2, sb)
//   stage 2: A  = perm(x2, x0, ta)  C  = perm(x2, x0, tc)  B  = perm(x3, x1, ta)  D  = perm(x3, x1, tc)
// Stage 2 is an involution (the way back uses ta, tc again); stage 1 is undone with va, vb.
// The table (one 32-byte row per action, game2048_env.py:196: 0 up, 1 right, 2 down, 3 left) is
// derived and checked by tests/test_device_math_host.py::test_move_lut.  The kernels keep it in LDS
// and fetch a lane's row with two ds_read (no VALU); the host check indexes the array directly.
struct MoveSel {
    uint32_t sa, sb, ta, tc, va, vb;
};

#define G2048_MOVE_LUT_WORDS                                                                        \
    0x03020100u, 0x07060504u, 0x03020100u, 0x07060504u, 0x03020100u, 0x07060504u, 0u, 0u, /* up */     \
    0x05010703u, 0x04000602u, 0x05040100u, 0x07060302u, 0x00040206u, 0x01050307u, 0u, 0u, /* right */  \
    0x07060504u, 0x03020100u, 0x07060504u, 0x03020100u, 0x07060504u, 0x03020100u, 0u, 0u, /* down */   \
    0x06020400u, 0x07030501u, 0x05040100u, 0x07060302u, 0x06020400u, 0x07030501u, 0u, 0u  /* left */

// game2048_env.py:194-241 with the lane's selector row.  Returns true when the board changed.
G2048_DEV bool move_sel(Board &bd, const MoveSel &s, uint32_t &score)
{
    const uint32_t x0 = g2048_perm(bd.r[1], bd.r[0], s.sa), x1 = g2048_perm(bd.r[1], bd.r[0], s.sb);
    const uint32_t x2 = g2048_perm(bd.r[3], bd.r[2], s.sa), x3 = g2048_perm(bd.r[3], bd.r[2], s.sb);
    uint32_t a = g2048_perm(x2, x0, s.ta), c = g2048_perm(x2, x0, s.tc);
    uint32_t b = g2048_perm(x3, x1, s.ta), d = g2048_perm(x3, x1, s.tc);
    const uint32_t a0 = a, b0 = b, c0 = c, d0 = d;
    score = shift4(a, b, c, d);
    const bool changed = ((a ^ a0) | (b ^ b0) | (c ^ c0) | (d ^ d0)) != 0; // :222,234,238
    const uint32_t y0 = g2048_perm(c, a, s.ta), y2 = g2048_perm(c, a, s.tc);
    const uint32_t y1 = g2048_perm(d, b, s.ta), y3 = g2048_perm(d, b, s.tc);
    bd.r[0] = g2048_perm(y1, y0, s.va);
    bd.r[1] = g2048_perm(y1, y0, s.vb);
    bd.r[2] = g2048_perm(y3, y2, s.va);
    bd.r[3] = g2048_perm(y3, y2, s.vb);
    return changed;
}

// ------------------------------------------------------------------------- expectimax search
// g2048_expectimax (include/g2048.h).  Everything is an integer, so every split of the tree across
// lanes gives the same bits.  For a line L = (a0, a1, a2, a3) (a row left to right or a column top to bottom):
//   empty(L) = #{a_i = 0}, merge(L) = #{i < 3 : a_i = a_{i+1} != 0},
//   inc(L) = sum over a_i <= a_{i+1} of a_i + a_{i+1}, dec(L) the same over a_i >= a_{i+1}, mono(L) = max(inc, dec);
//   H(b) = base + sum over the 8 lines of w_empty * empty + w_merge * merge + w_mono * mono          (< 2^27)
//   V_0 = H;  V_d(b) = max over legal m of C_d(move(b, m)), 0 when no move is legal;
//   C_d(a) = floor(sum over empty c of (9 V_{d-1}(a, c = 1) + V_{d-1}(a, c = 2)) / (10 E(a)))        (sum < 2^35)
// Exponents may reach 34 (31 + three merges): every byte stays below 0x80 and a line's inc / dec below 256.
struct SearchWeights {
    uint32_t base, w_empty, w_merge, w_mono;
};
constexpr uint32_t kSearchBase = 4096, kSearchEmpty = 256, kSearchMerge = 128, kSearchMono = 16; // = G2048_SEARCH_* (g2048.h)

// Four lines at once (byte l of a, b, c, d = 1st .. 4th cell of line l): merge pairs and sum of mono over the lines.
G2048_DEV void line_terms(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t &merges, uint32_t &mono)
{
    const uint32_t eab = z80(a ^ b) & nz80(a), ebc = z80(b ^ c) & nz80(b), ecd = z80(c ^ d) & nz80(c);
    merges += g2048_popc(eab | (ebc >> 1) | (ecd >> 2));
    // x <= y per byte: ((y | 0x80) - x) keeps bit 7 (no byte borrows, all bytes < 0x80)
    const uint32_t ab = a + b, bc = b + c, cd = c + d; // <= 68 per byte
    const uint32_t le_ab = mask7(((b | kHigh1) - a) & kHigh1), ge_ab = mask7(((a | kHigh1) - b) & kHigh1);
    const uint32_t le_bc = mask7(((c | kHigh1) - b) & kHigh1), ge_bc = mask7(((b | kHigh1) - c) & kHigh1);
    const uint32_t le_cd = mask7(((d | kHigh1) - c) & kHigh1), ge_cd = mask7(((c | kHigh1) - d) & kHigh1);
    const uint32_t inc = (ab & le_ab) + (bc & le_bc) + (cd & le_cd); // <= 204 per byte: no carry out of a byte
    const uint32_t dec = (ab & ge_ab) + (bc & ge_bc) + (cd & ge_cd);
    // max per line in 16-bit fields (the byte trick of max4 needs values below 0x80)
    const uint32_t ie = inc & 0x00ff00ffu, io = (inc >> 8) & 0x00ff00ffu;
    const uint32_t de = dec & 0x00ff00ffu, dv = (dec >> 8) & 0x00ff00ffu;
    const uint32_t ge_e = ((ie | 0x80008000u) - de) & 0x80008000u, ge_o = ((io | 0x80008000u) - dv) & 0x80008000u;
    const uint32_t s = bfi(ge_e - (ge_e >> 15), ie, de) + bfi(ge_o - (ge_o >> 15), io, dv);
    mono += (s & 0xffffu) + (s >> 16);
}

G2048_DEV uint32_t heuristic(const Board &bd, const SearchWeights &w)
{
    uint32_t merges = 0, mono = 0;
    line_terms(bd.r[0], bd.r[1], bd.r[2], bd.r[3], merges, mono); // columns: byte l of r[i] = cell (i, l)
    const Board t = transpose(bd);
    line_terms(t.r[0], t.r[1], t.r[2], t.r[3], merges, mono);     // rows
    return w.base + w.w_empty * (2u * count_empty(bd)) + w.w_merge * merges + w.w_mono * mono;
}

// Empty cells as a bit set: bit 8j + i for cell (i, j) -- register i, byte j.
G2048_DEV uint32_t empty_bits(const Board &bd)
{
    return (z80(bd.r[0]) >> 7) | (z80(bd.r[1]) >> 6) | (z80(bd.r[2]) >> 5) | (z80(bd.r[3]) >> 4);
}

// `bd` with exponent v in the empty cell of bit p (of empty_bits)
G2048_DEV Board place(const Board &bd, uint32_t p, uint32_t v)
{
    const uint32_t tile = v << (p & 24u), i = p & 7u;
    return Board{{bd.r[0] | (i == 0u ? tile : 0u), bd.r[1] | (i == 1u ? tile : 0u), bd.r[2] | (i == 2u ? tile : 0u),
                  bd.r[3] | (i == 3u ? tile : 0u)}};
}

template <int D, class Tables> G2048_DEV uint32_t search_value(const Board &bd, const SearchWeights &w, const Tables &tb);

// The chance items t = sub, sub + K, ... of the 2E items of afterstate `a` (item t = empty cell t / 2 in bit order, spawn
// exponent 1 + t % 2 with weight 9 / 1): f(child board, weight) for each.  K lanes with sub = 0 .. K-1 cover all items.
// The one item walk of both searches (chance_partial here, ntuple_chance_partial below).
template <class F> G2048_DEV void chance_items(const Board &a, uint32_t sub, uint32_t K, F &&f)
{
    uint32_t m = empty_bits(a), skipped = 0;
    const uint32_t items = 2u * g2048_popc(m);
#pragma unroll 1
    for (uint32_t t = sub; t < items; t += K) {
#pragma unroll 1
        for (; skipped < (t >> 1); ++skipped)
            m &= m - 1u;
        const uint32_t v = 1u + (t & 1u);
        f(place(a, g2048_ctz(m), v), v == 1u ? 9u : 1u);
    }
}

// Part of the chance-node sum of afterstate `a`: the items sub, sub + K, ... (chance_items).
template <int D, class Tables>
G2048_DEV uint64_t chance_partial(const Board &a, uint32_t sub, uint32_t K, const SearchWeights &w, const Tables &tb)
{
    uint64_t sum = 0;
    chance_items(a, sub, K, [&](const Board &child, uint32_t weight) {
        sum += static_cast<uint64_t>(weight) * search_value<D - 1>(child, w, tb);
    });
    return sum;
}

// C_D(a); a must have an empty cell
template <int D, class Tables> G2048_DEV uint32_t chance_value(const Board &a, const SearchWeights &w, const Tables &tb)
{
    return static_cast<uint32_t>(chance_partial<D>(a, 0u, 1u, w, tb) / (10u * count_empty(a)));
}

// V_D(b): the move selectors come from `tb` (LDS rows on the device) with a run-time index, so the four moves are one
// loop body and the depths D .. 1 one inlined body each -- no recursion and no per-lane array at run time.
template <int D, class Tables> G2048_DEV uint32_t search_value(const Board &bd, const SearchWeights &w, const Tables &tb)
{
    if constexpr (D == 0) {
        return heuristic(bd, w);
    } else {
        uint32_t best = 0;
#pragma unroll 1
        for (uint32_t m = 0; m < 4u; ++m) {
            Board a = bd;
            uint32_t gain;
            if (move_sel(a, tb.move_sel(m), gain)) {
                const uint32_t c = chance_value<D>(a, w, tb);
                best = c > best ? c : best;
            }
        }
        return best;
    }
}

// Root choice as one unsigned max: (value + 1) << 2 orders by value (illegal -1 lowest), 3 - m breaks ties to the
// smallest m.  KEY is as wide as the value: uint32_t for expectimax (value < 2^27), uint64_t for the rollout search
// (value < 2^62).  best_action: the action of the largest of the four keys, what the kernels find with two shuffles.
template <class KEY, class V> G2048_DEV KEY root_key(V value, uint32_t m) { return (static_cast<KEY>(value + 1) << 2) | (3u - m); }
template <class KEY> G2048_DEV uint32_t root_key_action(KEY key) { return 3u - (static_cast<uint32_t>(key) & 3u); }

template <class KEY, class V> G2048_DEV uint32_t best_action(const V value[4])
{
    KEY best = 0;
    for (uint32_t m = 0; m < 4u; ++m) {
        const KEY key = root_key<KEY>(value[m], m);
        best = key > best ? key : best;
    }
    return root_key_action(best);
}

// The root: value[m] = C_D(move(b, m)) or -1 when m is illegal, action = the smallest m with the largest value (0 when
// no move is legal).  One thread; the kernels split the same sums across lanes (chance_partial).
template <int D, class Tables>
G2048_DEV uint32_t search_root(const Board &cells, const SearchWeights &w, const Tables &tb, int32_t value[4])
{
    for (uint32_t m = 0; m < 4u; ++m) {
        Board a = cells;
        uint32_t gain;
        value[m] = move_sel(a, tb.move_sel(m), gain) ? static_cast<int32_t>(chance_value<D>(a, w, tb)) : -1;
    }
    return best_action<uint32_t>(value);
}

// ------------------------------------------------------------------- Monte-Carlo rollout search
// g2048_mc_search (include/g2048.h): try each root move, finish the game at random R times, take the
// move with the largest total score.  Integers only.  For board index i, root direction d, playout r, playout move j:
//   block(i, d, r, j) = Philox4x32-10(ctr = (j, r, i, d), key = (seed_lo, seed_hi ^ kMcKeyTag))
//   playout: a = move(b, d) (gain g; an illegal d has no playouts); total = g; then for j = 0, 1, ...: stop when j == L
//   (before the spawn: a spawn nobody moves on is not drawn); add_tile(a, block[0]); a0 = block[1] >> 30; play the first
//   of a0, a0 + 1, a0 + 2, a0 + 3 (mod 4) that is legal and add its merge score, or stop when none is (terminal).
//   value[d] = sum over r < R of total, steps[d] = sum over r of the moves played after the root move (-1: d illegal).
// A sum of pure functions of (i, d, r): every split of the playouts across lanes, in any order, gives the same bits.
// The per-move score is shift4's: the true merge score while it stays below 2^31, which holds for every board whose
// exponents are <= 26 (a move merges at most 8 pairs, each into an exponent <= 27: 8 * 2^27 = 2^30).  Above that it is
// the sum of 2^(e mod 32) over the merged cells with bit 31 dropped -- not the game's score, but the same on host and
// device, which share this code.
//
// The playout is phrased as a state machine that advances by ONE candidate move per trip (mc_trip), so that the kernel
// can run the lanes of a wave through one flat loop in which each lane is at its own playout, move and candidate: a
// lane whose candidate is illegal tries the next direction on its next trip, a lane whose playout ends starts its next
// playout on its next trip.  mc_playout / mc_root below are the same trips in sequence on one thread.
constexpr uint32_t kMcKeyTag = 0x4D435332u; // separates this stream from the engine's spawn stream under an equal seed
constexpr uint32_t kMcMaxRollouts = 65536, kMcMaxSteps = 65535; // = G2048_MC_MAX_* (g2048.h): steps sums fit 32 bits per lane

struct McPlayout {
    Board a;        // the playout's board: after a move, before the spawn that answers it
    uint32_t moves; // moves played after the root move = index j of the next Philox block
    uint32_t tries; // candidates of the current move already found illegal (0: the spawn is still to be drawn)
};

G2048_DEV McPlayout mc_begin(const Board &after) { return McPlayout{after, 0u, 0u}; }

// One trip: draws the spawn when this is the move's first candidate, tries candidate (a0 + tries) mod 4.  Adds the merge
// score of a legal move to `total` and 1 to `steps`.  Returns true when the playout has ended (cap or terminal).
// i, d, r: board index, root direction, playout; max_steps = L >= 1.
template <class Tables>
G2048_DEV bool mc_trip(McPlayout &p, uint32_t i, uint32_t d, uint32_t r, uint32_t seed_lo, uint32_t seed_hi,
                       uint32_t max_steps, const Tables &tb, uint64_t &total, uint32_t &steps)
{
    // the block of move j = p.moves; a retry recomputes it (cheaper than keeping four words live per lane)
    const Words w = philox4x32_10(p.moves, r, i, d, seed_lo, seed_hi ^ kMcKeyTag);
    add_tile(p.a, w.w[0], lanemask(p.tries == 0u));
    Board b = p.a;
    uint32_t gain;
    const bool legal = move_sel(b, tb.move_sel(((w.w[1] >> 30) + p.tries) & 3u), gain);
    if (legal) {
        p.a = b;
        total += gain;
        steps += 1u;
        p.moves += 1u;
        p.tries = 0u;
        return p.moves == max_steps; // the cap, before the next spawn
    }
    p.tries += 1u;
    return p.tries == 4u;            // no candidate is legal: terminal
}

// One whole playout from the root afterstate `after` (gain g already counted by the caller).
template <class Tables>
G2048_DEV void mc_playout(const Board &after, uint32_t i, uint32_t d, uint32_t r, uint32_t seed_lo, uint32_t seed_hi,
                          uint32_t max_steps, const Tables &tb, uint64_t &total, uint32_t &steps)
{
    McPlayout p = mc_begin(after);
    while (!mc_trip(p, i, d, r, seed_lo, seed_hi, max_steps, tb, total, steps)) {
    }
}

// The playouts sub, sub + K, ... (< R) of root direction d: what one lane of the kernel sums.  `after`, g: move(b, d).
template <class Tables>
G2048_DEV void mc_partial(const Board &after, uint32_t g, uint32_t i, uint32_t d, uint32_t sub, uint32_t K, uint32_t rollouts,
                          uint32_t seed_lo, uint32_t seed_hi, uint32_t max_steps, const Tables &tb, uint64_t &total, uint64_t &steps)
{
    for (uint32_t r = sub; r < rollouts; r += K) {
        uint32_t s = 0;
        total += g;
        mc_playout(after, i, d, r, seed_lo, seed_hi, max_steps, tb, total, s);
        steps += s;
    }
}

// The root on one thread: value[4], steps[4] (-1 where d is illegal) and the action (smallest d of largest value, 0
// when no move is legal).
template <class Tables>
G2048_DEV uint32_t mc_root(const Board &cells, uint32_t i, uint32_t rollouts, uint32_t max_steps, uint32_t seed_lo,
                           uint32_t seed_hi, const Tables &tb, int64_t value[4], int64_t steps[4])
{
    for (uint32_t d = 0; d < 4u; ++d) {
        Board after = cells;
        uint32_t g;
        value[d] = steps[d] = -1;
        if (move_sel(after, tb.move_sel(d), g)) {
            uint64_t total = 0, st = 0;
            mc_partial(after, g, i, d, 0u, 1u, rollouts, seed_lo, seed_hi, max_steps, tb, total, st);
            value[d] = static_cast<int64_t>(total);
            steps[d] = static_cast<int64_t>(st);
        }
    }
    return best_action<uint64_t>(value);
}

// ------------------------------------------------------------------- n-tuple network value function
// g2048_ntuple_* (include/g2048.h): a value function that is nothing but table look-ups, learned by
// afterstate TD(0) (Szubert & Jaskowski 2014).  T tuples of L cells each; tuple t owns a table of 16^L int32 weights, a
// weight being a score in units of 2^-F.  Integers only:
//   c(e)     = min(e mod 32, 15)                              (tiles of 2^15 and above share the last table row)
//   idx_t(b) = sum over k < L of c(b[cells[t][k]]) << 4k
//   V(b)     = sum over the 8 symmetries s of b, sum over t < T of weights[t][idx_t(s(b))]             (|V| <= 2^37)
//   evaluate: q[d] = (g_d << F) + V(a_d) for (a_d, g_d) = move(b, d), kNtupleIllegal where d is illegal; action = the
//             smallest d of largest q (q may be negative), 0 when no move is legal; best = q[action], after = a_action,
//             after_value = V(after) -- 0, the input board, 0 when no move is legal
//   update:   step = sat_int32(delta >> lr_shift) (arithmetic shift); weights[t][idx_t(s(a))] += step for every s and t,
//             a 32-bit add that wraps.  A sum of adds: any order, any split over lanes or launches gives the same weights.
// The symmetries are applied to the CELL LISTS, once, on the host: s(b)[c] = b[ntuple_sym_cell(s, c)], so
// idx_t(s(b)) reads b at the cells ntuple_sym_cell(s, cells[t][k]) -- NtupleShape::list holds those 8T lists as six
// nibbles each.  The lists are wave-uniform kernel arguments (SGPRs), the board is its 16 clamped cells packed into one
// 64-bit value, and reading a cell is a 64-bit shift by a scalar amount: no per-lane array, nothing in scratch.  The eight
// maps (transpose, reverse the rows, reverse the columns, in every combination) are the dihedral group of the square, the
// set training_data.augment() / g2048_augment generate; the sum does not care about their order.
#if defined(G2048_HOST_CHECK)
#define G2048_HOST_DEV static inline
#define G2048_MEMBER inline // a member function, for device code and for the launcher
#else
#define G2048_HOST_DEV __host__ __device__ __forceinline__
#define G2048_MEMBER __host__ __device__ __forceinline__
#endif
constexpr uint32_t kNtupleMaxTuples = 8, kNtupleMaxLen = 6, kNtupleMaxFrac = 16, kNtupleMaxShift = 40; // = G2048_NTUPLE_* (g2048.h)
constexpr int64_t kNtupleIllegal = INT64_MIN;                                                          // G2048_NTUPLE_ILLEGAL

// Multi-stage networks (g2048_ntuple_staged_*, include/g2048.h; Yeh et al. 2016, Jaskowski 2017): S
// weight sets [S][T][16^L], the set of a board chosen by the tiles it holds.  Integers only, a function of the board alone:
//   mask(b)  = OR over the 16 cells of 1 << c(b[cell])        (16 bits; bit 0 = "has an empty cell"; the same for all 8 symmetries)
//   stage(b) = the number of j < S - 1 with mask(b) >= thr[j]  (thr strictly ascending, 1..65535; compared as integers)
//   off(b, s, t) = (stage(b) * T + t) * 16^L + idx_t(s(b))     (an element index below 2^30; the BYTE offset needs 64 bits)
// Every definition of this header reads and writes the tables of stage(board it looks up): the four afterstates of a board,
// the leaves below a chance node and the slots of a trace history may all sit in different stages, and stage(b) is not
// monotone over a game (16k + 8k + 8k -> 16k + 16k leaves the stage of 0x6000).  S = 1 is the network of above, bit for bit.
// The stages are a compile-time property of a kernel: the unstaged entry points pass an NtupleShape, exactly the kernel
// argument they had before stages existed, and compute no mask; a network with S > 1 passes an NtupleStagedShape.  Every
// per-board function below is a template on the shape type (deduced), and ntuple_stage_base is the one place that differs.
// NtupleStagedShape::thr holds kNtupleNoStage, which no mask reaches, from entry S - 1 on: stage() needs no S.
constexpr uint32_t kNtupleMaxStages = 8;          // = G2048_NTUPLE_MAX_STAGES (g2048.h)
constexpr uint32_t kNtupleNoStage = 0x10000u;     // above every 16-bit mask

struct NtupleShape {
    uint32_t n_tuples, tuple_len;
    uint32_t list[8 * kNtupleMaxTuples]; // list[8 * s + t]: nibble k = the cell of b that idx_t(s(b)) reads for k
};
struct NtupleStagedShape : NtupleShape {
    uint32_t thr[kNtupleMaxStages - 1];  // thr[j], j < S - 1; kNtupleNoStage from there on
};

// Mixed-length networks (redundant encoding, Jaskowski 2017; include/g2048.h): a cell list may end before
// tuple_len with kNtupleEnd entries, tuple t then has L_t cells and a table of 16^L_t weights, and the tables lie back to back:
//   base_t = sum over u < t of 16^L_u,   W = sum over t of 16^L_t,   off(b, s, t) = stage(b) * W + base_t + idx_t(s(b))
// with idx_t summed over k < L_t.  Still an element index below 2^30 (7 * 8 * 16^6), and every table starts on a multiple of
// 16 elements.  A third shape type beside the two above, so the uniform kernels keep their arguments and their code: the
// list words are NtupleShape's with 4 * L_t in the top byte (an END entry reads cell 0 and is masked off the index), and the
// type carries the thresholds too -- an unstaged mixed network has kNtupleNoStage in all seven and is stage 0.
constexpr uint32_t kNtupleEnd = 0xffu; // = G2048_NTUPLE_END (g2048.h)
struct NtupleMixedShape {
    uint32_t n_tuples, n_weights;        // T, W
    uint32_t list[8 * kNtupleMaxTuples]; // list[8 * s + t]: bits 0..23 as NtupleShape::list, bits 24..31 = 4 * L_t
    uint32_t base[kNtupleMaxTuples];     // base_t
    uint32_t thr[kNtupleMaxStages - 1];  // as NtupleStagedShape::thr
};

// The cell of b that symmetry s (0..7) puts at cell c: bit 0 transposes, bit 1 reverses the rows, bit 2 the columns.
G2048_HOST_DEV uint32_t ntuple_sym_cell(uint32_t s, uint32_t c)
{
    uint32_t r = c >> 2, q = c & 3u;
    if (s & 1u) {
        const uint32_t x = r;
        r = q;
        q = x;
    }
    if (s & 2u)
        r = 3u - r;
    if (s & 4u)
        q = 3u - q;
    return 4u * r + q;
}

G2048_HOST_DEV NtupleShape ntuple_shape(uint32_t n_tuples, uint32_t tuple_len, const uint8_t cells[8][6])
{
    NtupleShape sh{};
    sh.n_tuples = n_tuples;
    sh.tuple_len = tuple_len;
    for (uint32_t s = 0; s < 8u; ++s)
        for (uint32_t t = 0; t < n_tuples; ++t)
            for (uint32_t k = 0; k < tuple_len; ++k)
                if (cells[t][k] != kNtupleEnd)
                    sh.list[8u * s + t] |= ntuple_sym_cell(s, cells[t][k]) << (4u * k);
    return sh;
}

// thresholds: the n_stages - 1 ascending thresholds of a staged network
G2048_HOST_DEV NtupleStagedShape ntuple_staged_shape(const NtupleShape &shape, uint32_t n_stages, const uint16_t *thresholds)
{
    NtupleStagedShape sh{};
    static_cast<NtupleShape &>(sh) = shape;
    for (uint32_t j = 0; j < kNtupleMaxStages - 1u; ++j)
        sh.thr[j] = j + 1u < n_stages ? thresholds[j] : kNtupleNoStage;
    return sh;
}

// L_t of a checked descriptor: the entries before the first kNtupleEnd among k < tuple_len
G2048_HOST_DEV uint32_t ntuple_tuple_len(uint32_t tuple_len, const uint8_t cells[6])
{
    uint32_t len = 0;
    while (len < tuple_len && cells[len] != kNtupleEnd)
        ++len;
    return len;
}

// whether a checked descriptor is a mixed network: some list ends before tuple_len
G2048_HOST_DEV bool ntuple_is_mixed(uint32_t n_tuples, uint32_t tuple_len, const uint8_t cells[8][6])
{
    for (uint32_t t = 0; t < n_tuples; ++t)
        if (ntuple_tuple_len(tuple_len, cells[t]) != tuple_len)
            return true;
    return false;
}

// thresholds: as ntuple_staged_shape takes them; n_stages = 1 for a network of one weight set
G2048_HOST_DEV NtupleMixedShape ntuple_mixed_shape(uint32_t n_tuples, uint32_t tuple_len, const uint8_t cells[8][6], uint32_t n_stages,
                                                   const uint16_t *thresholds)
{
    const NtupleShape lists = ntuple_shape(n_tuples, tuple_len, cells);
    NtupleMixedShape sh{};
    sh.n_tuples = n_tuples;
    for (uint32_t t = 0; t < n_tuples; ++t) {
        const uint32_t len = ntuple_tuple_len(tuple_len, cells[t]);
        sh.base[t] = sh.n_weights;
        sh.n_weights += 1u << (4u * len);
        for (uint32_t s = 0; s < 8u; ++s)
            sh.list[8u * s + t] = lists.list[8u * s + t] | (4u * len) << 24;
    }
    for (uint32_t j = 0; j < kNtupleMaxStages - 1u; ++j)
        sh.thr[j] = j + 1u < n_stages ? thresholds[j] : kNtupleNoStage;
    return sh;
}

// mask(b) of a packed board (ntuple_pack: the 16 clamped cells as nibbles)
G2048_HOST_DEV uint32_t ntuple_stage_mask(uint64_t packed)
{
    uint32_t mask = 0;
    for (uint32_t c = 0; c < 16u; ++c)
        mask |= 1u << (static_cast<uint32_t>(packed >> (4u * c)) & 15u);
    return mask;
}

// stage(b) for mask = mask(b): 0..S-1; Shape = NtupleStagedShape or NtupleMixedShape
template <class Shape> G2048_HOST_DEV uint32_t ntuple_stage(uint32_t mask, const Shape &sh)
{
    uint32_t stage = 0;
    for (uint32_t j = 0; j < kNtupleMaxStages - 1u; ++j)
        stage += mask >= sh.thr[j] ? 1u : 0u;
    return stage;
}

// c(e) for the four cells of a row register: min(byte mod 32, 15)
G2048_DEV uint32_t ntuple_cell(uint32_t row)
{
    const uint32_t e = row & 0x1f1f1f1fu;
    const uint32_t over = (e >> 4) & 0x01010101u; // 1 where the exponent is 16..31
    return (e | (over * 15u)) & 0x0f0f0f0fu;
}

// The 16 clamped cells as nibbles: cell c in bits 4c .. 4c + 3
G2048_DEV uint64_t ntuple_pack(const Board &b)
{
    uint32_t h[4];
    for (int i = 0; i < 4; ++i) {
        uint32_t x = ntuple_cell(b.r[i]);
        x = (x | (x >> 4)) & 0x00ff00ffu;
        h[i] = (x | (x >> 8)) & 0xffffu;
    }
    return (static_cast<uint64_t>(h[2] | (h[3] << 16)) << 32) | (h[0] | (h[1] << 16));
}

// idx of one cell list (six nibbles, the first L used) on a packed board; < 16^L
G2048_DEV uint32_t ntuple_index(uint64_t packed, uint32_t list, uint32_t L)
{
    uint32_t idx = 0;
#pragma unroll
    for (uint32_t k = 0; k < kNtupleMaxLen; ++k) {
        const uint32_t cell = (list >> (4u * k)) & 15u;
        idx |= (static_cast<uint32_t>(packed >> (4u * cell)) & (k < L ? 15u : 0u)) << (4u * k);
    }
    return idx;
}

// stage(b) * T * 16^L, the element offset of the board's weight set in [S][T][16^L]: once per packed board, before its 8T
// offsets.  At most 7 * 8 * 16^6 < 2^30.  The unstaged shape has one set: a constant 0 that folds away.
G2048_DEV uint32_t ntuple_stage_base(uint64_t, const NtupleShape &) { return 0u; }
G2048_DEV uint32_t ntuple_stage_base(uint64_t packed, const NtupleStagedShape &sh)
{
    return (ntuple_stage(ntuple_stage_mask(packed), sh) * sh.n_tuples) << (4u * sh.tuple_len);
}
// stage(b) * W of a mixed network, at most 7 * 8 * 16^6 < 2^30
G2048_DEV uint32_t ntuple_stage_base(uint64_t packed, const NtupleMixedShape &sh)
{
    return ntuple_stage(ntuple_stage_mask(packed), sh) * sh.n_weights;
}

// offset of look-up (s, t) of a board whose weight set starts at element `base` (ntuple_stage_base) in the weight array
// [S][T][16^L]; < S * T * 16^L <= 2^30: an ELEMENT index that fits uint32.  Every user adds it to a 64-bit pointer (the
// byte offset of S = 8, T = 8, L = 6 reaches 4 GiB in the weights and 8 GiB in a TC accumulator).
G2048_DEV uint32_t ntuple_offset(uint64_t packed, const NtupleShape &sh, uint32_t s, uint32_t t, uint32_t base)
{
    return base + (t << (4u * sh.tuple_len)) + ntuple_index(packed, sh.list[8u * s + t], sh.tuple_len);
}
// the same in a mixed network, < S * W <= 2^30: the index over all six nibbles, cut to the 4 * L_t bits of the list's top byte
G2048_DEV uint32_t ntuple_offset(uint64_t packed, const NtupleMixedShape &sh, uint32_t s, uint32_t t, uint32_t base)
{
    const uint32_t list = sh.list[8u * s + t];
    return base + sh.base[t] + (ntuple_index(packed, list, kNtupleMaxLen) & ((1u << (list >> 24)) - 1u));
}

// V(b), read from the tables of stage(b).  T = sh.n_tuples as a template argument: the 8T look-ups are straight-line code,
// the stage base and all offsets first, then all loads, then the adds -- the loads do not depend on each other and are in
// flight together.
template <uint32_t T, class Shape> G2048_DEV int64_t ntuple_value(uint64_t packed, const Shape &sh, const int32_t *weights)
{
    uint32_t off[8u * T];
    int32_t w[8u * T];
    const uint32_t base = ntuple_stage_base(packed, sh);
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s)
#pragma unroll
        for (uint32_t t = 0; t < T; ++t)
            off[s * T + t] = ntuple_offset(packed, sh, s, t, base);
#pragma unroll
    for (uint32_t j = 0; j < 8u * T; ++j)
        w[j] = weights[off[j]];
    int64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u * T; ++j)
        v += w[j];
    return v;
}

// One root direction: the afterstate, its value and q.
struct NtupleMove {
    Board after;
    int64_t v, q; // V(after); (gain << F) + v, kNtupleIllegal where the move is illegal
    bool legal;
};

template <uint32_t T, class Shape, class Tables>
G2048_DEV NtupleMove ntuple_move(const Board &cells, uint32_t d, const Shape &sh, uint32_t F, const int32_t *weights,
                                 const Tables &tb)
{
    NtupleMove m;
    m.after = cells;
    uint32_t gain;
    m.legal = move_sel(m.after, tb.move_sel(d), gain); // illegal: after == cells
    m.v = ntuple_value<T>(ntuple_pack(m.after), sh, weights);
    m.q = m.legal ? static_cast<int64_t>(static_cast<uint64_t>(gain) << F) + m.v : kNtupleIllegal;
    return m;
}

// Root choice as one unsigned max.  |q| < 2^48 (gain < 2^31, F <= 16, |V| <= 2^37), so q + 2^60 is positive and fits 62
// bits: a signed-to-unsigned bias (root_key's value + 1 assumes values >= -1).  An illegal direction's key is below
// every legal one; 3 - d breaks ties to the smallest d and makes the action 0 when no direction is legal.
G2048_DEV uint64_t ntuple_key(int64_t q, bool legal, uint32_t d)
{
    return (legal ? static_cast<uint64_t>(q + (1ll << 60)) << 2 : 0ull) | (3u - d);
}
G2048_DEV bool ntuple_key_legal(uint64_t key) { return key >= 4u; }

// The evaluate definition on one thread; the kernel gives each direction a lane and joins the keys with two shuffles.
struct NtupleRoot {
    int64_t q[4];
    uint32_t action;
    int64_t best;
    Board after;
    int64_t after_value;
};

template <uint32_t T, class Shape, class Tables>
G2048_DEV NtupleRoot ntuple_root(const Board &cells, const Shape &sh, uint32_t F, const int32_t *weights, const Tables &tb)
{
    NtupleRoot r;
    NtupleMove m[4];
    uint64_t best = 0;
    for (uint32_t d = 0; d < 4u; ++d) {
        m[d] = ntuple_move<T>(cells, d, sh, F, weights, tb);
        r.q[d] = m[d].q;
        const uint64_t key = ntuple_key(m[d].q, m[d].legal, d);
        best = key > best ? key : best;
    }
    r.action = root_key_action(best);
    const bool any = ntuple_key_legal(best);
    r.best = any ? r.q[r.action] : 0;
    r.after = any ? m[r.action].after : cells;
    r.after_value = any ? m[r.action].v : 0;
    return r;
}

// The update's step: sat_int32(delta >> lr_shift), the shift arithmetic (it floors negatives); lr_shift <= 40
G2048_DEV int32_t ntuple_step(int64_t delta, uint32_t lr_shift)
{
    const int64_t x = delta >> lr_shift;
    return x > INT32_MAX ? INT32_MAX : (x < INT32_MIN ? INT32_MIN : static_cast<int32_t>(x));
}

// add(offset, step) for each of the 8T look-ups of one board: the device passes a fire-and-forget atomic, the host a
// wrapping add.
template <uint32_t T, class Shape, class Add> G2048_DEV void ntuple_update(uint64_t packed, const Shape &sh, int32_t step, Add add)
{
    const uint32_t base = ntuple_stage_base(packed, sh);
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s)
#pragma unroll
        for (uint32_t t = 0; t < T; ++t)
            add(ntuple_offset(packed, sh, s, t, base), step);
}

// Temporal-coherence learning (g2048_ntuple_tc_update_plain, include/g2048.h; Beal & Smith 1999,
// Jaskowski 2017): every weight has two int64 accumulators, err = E (the signed sum of the deltas it has seen) and
// mag = A (the sum of their magnitudes, an unsigned 64-bit number), and learns at its own rate |E| / A.  Integers only:
//   rate(E, A)  A == 0 -> 65536 (1.0 in Q16); else m = min(|E| as uint64, A), k = max(0, bitlen(A) - 32),
//               r = floor(((m >> k) << 16) / (A >> k)), 0..65536
//   d           = clamp(delta, -2^40, +2^40)
//   step(d, r)  = sat_int32((d * r) >> (16 + lr_shift)), the shift arithmetic; |d * r| <= 2^56
//   phase W: weights[j] += step(d_i, rate(err[j], mag[j])) for each of the 8T look-ups j of board i, err and mag as they
//            were BEFORE the call;   phase A: err[j] += d_i, mag[j] += |d_i|.   d_i == 0 touches nothing.
// Phase W only reads the accumulators and phase A only adds to them, each in a launch of its own: sums of integer adds,
// the same bits in any lane order.  rate is total: any bit pattern of E and A gives a result in 0..65536.
constexpr int64_t kNtupleTcMaxDelta = 1ll << 40; // the clamp of d
constexpr uint32_t kNtupleTcOne = 1u << 16;      // rate 1.0

// floor((m << 16) / a) for m <= a, 1 <= a < 2^32: at most 65536.  The float estimate is off by less than 2^-6 -- two
// conversions and a product of half an ulp each, a reciprocal of at most 2.5 ulp, on a quotient of at most 2^16 -- so its
// floor is the quotient or a neighbour of it, and one step either way on the exact remainder lands on it.
G2048_DEV uint32_t ntuple_tc_quotient(uint32_t m, uint32_t a)
{
    const uint64_t num = static_cast<uint64_t>(m) << 16;
    uint32_t q = static_cast<uint32_t>(static_cast<float>(m) * 65536.0f * g2048_rcp(static_cast<float>(a)));
    const int64_t rem = static_cast<int64_t>(num - static_cast<uint64_t>(q) * a);
    q -= rem < 0 ? 1u : 0u;
    q += rem >= static_cast<int64_t>(a) ? 1u : 0u;
    return q;
}

G2048_DEV uint32_t ntuple_tc_rate(int64_t err, uint64_t mag)
{
    if (mag == 0)
        return kNtupleTcOne;
    const uint64_t e = err < 0 ? 0ull - static_cast<uint64_t>(err) : static_cast<uint64_t>(err); // INT64_MIN -> 2^63
    const uint64_t m = e < mag ? e : mag;
    const uint32_t hi = static_cast<uint32_t>(mag >> 32);
    const uint32_t k = hi ? 32u - g2048_clz(hi) : 0u; // bitlen(A) - 32 where that is positive
    return ntuple_tc_quotient(static_cast<uint32_t>(m >> k), static_cast<uint32_t>(mag >> k));
}

G2048_DEV int64_t ntuple_tc_delta(int64_t delta)
{
    return delta > kNtupleTcMaxDelta ? kNtupleTcMaxDelta : (delta < -kNtupleTcMaxDelta ? -kNtupleTcMaxDelta : delta);
}

// d as ntuple_tc_delta returns it, rate 0..65536, lr_shift <= 40
G2048_DEV int32_t ntuple_tc_step(int64_t d, uint32_t rate, uint32_t lr_shift)
{
    const int64_t x = (d * static_cast<int64_t>(rate)) >> (16u + lr_shift);
    return x > INT32_MAX ? INT32_MAX : (x < INT32_MIN ? INT32_MIN : static_cast<int32_t>(x));
}

// Phase W of one board, d != 0: all 8T offsets, then all 16T accumulator loads (independent: in flight together, as in
// ntuple_value), then the rates and steps, then add(offset, step) for every step that is not 0.
template <uint32_t T, class Shape, class Add>
G2048_DEV void ntuple_tc_weights(uint64_t packed, const Shape &sh, int64_t d, uint32_t lr_shift, const int64_t *err,
                                 const int64_t *mag, Add add)
{
    uint32_t off[8u * T];
    int64_t e[8u * T];
    uint64_t a[8u * T];
    const uint32_t base = ntuple_stage_base(packed, sh);
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s)
#pragma unroll
        for (uint32_t t = 0; t < T; ++t)
            off[s * T + t] = ntuple_offset(packed, sh, s, t, base);
#pragma unroll
    for (uint32_t j = 0; j < 8u * T; ++j) {
        e[j] = err[off[j]];
        a[j] = static_cast<uint64_t>(mag[off[j]]);
    }
#pragma unroll
    for (uint32_t j = 0; j < 8u * T; ++j) {
        const int32_t step = ntuple_tc_step(d, ntuple_tc_rate(e[j], a[j]), lr_shift);
        if (step != 0)
            add(off[j], step);
    }
}

// Phase A of one board, d != 0: add(offset, d, |d|) for each of the 8T look-ups.
template <uint32_t T, class Shape, class Add> G2048_DEV void ntuple_tc_accum(uint64_t packed, const Shape &sh, int64_t d, Add add)
{
    const uint64_t m = static_cast<uint64_t>(d < 0 ? -d : d);
    const uint32_t base = ntuple_stage_base(packed, sh);
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s)
#pragma unroll
        for (uint32_t t = 0; t < T; ++t)
            add(ntuple_offset(packed, sh, s, t, base), d, m);
}

// n-tuple traces (g2048_ntuple_trace_push / g2048_ntuple_trace_update / g2048_ntuple_tc_trace_update, include/g2048.h,
// INTEGRATION.md §12; Sutton 1988, the TC(lambda) of Jaskowski 2017): the error of step t also moves, decayed, the last
// few afterstates of the same board.  The history is caller-owned device memory, zero-initialised, one per engine or shard:
//   H     1..kNtupleTraceMax (= 8) slots
//   lam   lambda in Q16, 0..65536
//   hist  uint8 [H][n][16]   slot-major, 16-byte aligned: slot k of board i is the 16 exponents at hist + (k*n + i)*16
//   len   uint8 [n]          bits 0..6: number of valid slots; bit 7: the episode ended at the last push
// push(slot), for every board i, slot in 0..H-1 (the caller advances slot by one mod H before each push):
//   old      = len[i];   l = (old & 0x80) ? 0 : min(old & 0x7f, H)
//   hist[slot][i] = after[i]                                                   (16 bytes)
//   delta[i] = (terminated[i] ? 0 : best_next[i]) - after_value[i]             (int64, wraps; exactly td_evaluate's delta)
//   len[i]   = min(l + 1, H) | (terminated[i] ? 0x80 : 0)
// push is total: any byte in len gives a defined result.
// trace update(slot), slot the slot of the last push, for every board i:
//   L   = min(len[i] & 0x7f, H);   d = clamp(delta[i], -2^40, +2^40)           (ntuple_tc_delta)
//   p_0 = 65536;  p_k = (p_{k-1} * lam) >> 16                                  (uint64 arithmetic; 0..65536)
//   for k in 0..L-1:   a   = hist[(slot + H - k) mod H][i]
//                      d_k = (d * p_k) >> 16                                   (arithmetic shift: floors negatives; |d*p_k| <= 2^56)
//     TD:    step = ntuple_step(d_k, lr_shift);  weights[off(a,s,t)] += step for all s, t;  a zero step touches nothing
//     TC W:  weights[j] += ntuple_tc_step(d_k, rate(err[j], mag[j]), lr_shift)  with err, mag as they were before the call
//     TC A:  err[j] += d_k;  mag[j] += |d_k|                                    d_k == 0 touches nothing
// The same weight entry reached from two slots, or from two symmetries, counts once per reach.  Phase W and phase A are
// separate launches, as above and for the same reason.  The shifts floor: a negative d_k decays to -1 and not to 0, while
// its positive twin reaches 0 -- the rule ntuple_step and ntuple_tc_step follow.  With H = 1 or lam = 0 (p_k = 0 for
// k > 0) the TD form is the plain update whenever |delta| <= 2^40, and the TC form is the plain TC update always.
constexpr uint32_t kNtupleTraceMax = 8;        // = G2048_NTUPLE_TRACE_MAX (g2048.h)
constexpr uint32_t kNtupleTraceEnded = 0x80u;  // bit 7 of a len byte

// l of push: the valid slots an old len byte stands for -- none once the episode has ended
G2048_DEV uint32_t ntuple_trace_kept(uint32_t old, uint32_t H)
{
    const uint32_t l = old & 0x7fu;
    return (old & kNtupleTraceEnded) ? 0u : (l < H ? l : H);
}

// the len byte push writes
G2048_DEV uint32_t ntuple_trace_push_len(uint32_t old, uint32_t H, bool terminated)
{
    const uint32_t l = ntuple_trace_kept(old, H) + 1u;
    return (l < H ? l : H) | (terminated ? kNtupleTraceEnded : 0u);
}

// the delta push writes; the subtraction wraps mod 2^64
G2048_DEV int64_t ntuple_trace_delta(int64_t best_next, int64_t after_value, bool terminated)
{
    return static_cast<int64_t>((terminated ? 0ull : static_cast<uint64_t>(best_next)) - static_cast<uint64_t>(after_value));
}

// L of the update: min(len & 0x7f, H)
G2048_DEV uint32_t ntuple_trace_len(uint32_t len, uint32_t H)
{
    const uint32_t l = len & 0x7fu;
    return l < H ? l : H;
}

// p_k, k < kNtupleTraceMax, lam <= 65536: at most 65536, and never increasing in k
G2048_DEV uint32_t ntuple_trace_decay(uint32_t lam, uint32_t k)
{
    uint64_t p = kNtupleTcOne;
    for (uint32_t j = 0; j < k; ++j)
        p = (p * lam) >> 16;
    return static_cast<uint32_t>(p);
}

// d_k for d as ntuple_tc_delta returns it and p = p_k
G2048_DEV int64_t ntuple_trace_dk(int64_t d, uint32_t p) { return (d * static_cast<int64_t>(p)) >> 16; }

// the slot that holds the afterstate k pushes before the one in `slot`; k < H, slot < H
G2048_DEV uint32_t ntuple_trace_slot(uint32_t slot, uint32_t k, uint32_t H)
{
    const uint32_t s = slot + H - k;
    return s >= H ? s - H : s;
}

// Work item `item` < H * n of a trace update, k-major: item = k * n + i.  H <= 8, so k is a count of compares, not a
// 64-bit division.
G2048_DEV void ntuple_trace_split(uint64_t item, uint32_t n, uint32_t H, uint32_t &k, uint32_t &i)
{
    k = 0;
    for (uint32_t j = 1; j < H; ++j)
        k += item >= static_cast<uint64_t>(j) * n ? 1u : 0u;
    i = static_cast<uint32_t>(item - static_cast<uint64_t>(k) * n);
}

// One work item (k, i) of a trace update up to the point where it needs its board: d_k, or 0 when the item has nothing
// to do (k >= L, or d_k == 0).  len_i and delta_i are the item's only loads so far.
G2048_DEV int64_t ntuple_trace_item(uint32_t len_i, int64_t delta_i, uint32_t k, uint32_t H, uint32_t lam)
{
    if (k >= ntuple_trace_len(len_i, H))
        return 0;
    return ntuple_trace_dk(ntuple_tc_delta(delta_i), ntuple_trace_decay(lam, k));
}

// The work items of an update.  All six updates -- TD, TC phase W, TC phase A, each over plain boards or over a trace
// history -- are one loop over the items of a source (ntuple_for_items) and one per-item operation; the update kernels
// run exactly this with atomic adds, the host check of the tests with wrapping adds.  A source is a compile-time type, as
// the shape is: it says how many items there are, which delta an item sees -- without touching its board, so an item
// with nothing to do leaves before the 16-byte load -- and, on demand, the item's packed board.  `delta` is the int64 [n]
// array of the call, one entry per board; it is passed alongside the source so that a kernel can take it as a __restrict__
// argument of its own.
//   td_delta: what the TD step shifts.  Plain boards: delta[i] as it is (the one form that does not clamp); trace: d_k.
//   tc_delta: d of phase W and phase A.  Plain boards: clamp(delta[i]) (ntuple_tc_delta); trace: d_k.
struct NtupleBoardItems { // item i = board i
    const uint4 *boards;
    uint32_t n;
    using Item = uint32_t;
    G2048_MEMBER uint64_t size() const { return n; }
    G2048_MEMBER Item at(uint64_t index) const { return static_cast<uint32_t>(index); }
    G2048_MEMBER int64_t td_delta(const int64_t *delta, Item i) const { return delta[i]; }
    G2048_MEMBER int64_t tc_delta(const int64_t *delta, Item i) const { return ntuple_tc_delta(delta[i]); }
    G2048_MEMBER uint64_t packed(Item i) const { return ntuple_pack(load_board(boards, i)); }
};

// item k * n + i = the afterstate of board i that is k pushes old (ntuple_trace_split): k-major, so a wave reads 64
// consecutive boards of one slot.  The item index and the slot base are 64-bit: H * n * 16 bytes exceeds 2^32.
struct NtupleTraceItems {
    const uint4 *hist;  // [H][n] boards
    const uint8_t *len; // [n]
    uint32_t n, H, lam, slot; // slot: that of the last push
    struct Item {
        uint32_t k, i;
    };
    G2048_MEMBER uint64_t size() const { return static_cast<uint64_t>(H) * n; }
    G2048_MEMBER Item at(uint64_t index) const
    {
        Item it;
        ntuple_trace_split(index, n, H, it.k, it.i);
        return it;
    }
    G2048_MEMBER int64_t td_delta(const int64_t *delta, Item it) const
    {
        return ntuple_trace_item(len[it.i], delta[it.i], it.k, H, lam);
    }
    G2048_MEMBER int64_t tc_delta(const int64_t *delta, Item it) const { return td_delta(delta, it); }
    G2048_MEMBER uint64_t packed(Item it) const
    {
        return ntuple_pack(load_board(hist + static_cast<uint64_t>(ntuple_trace_slot(slot, it.k, H)) * n, it.i));
    }
};

// f(item) for the items first, first + stride, ... of a source: a lane of a kernel strides by the grid, the host by 1
template <class Items, class F> G2048_DEV void ntuple_for_items(const Items &items, uint64_t first, uint64_t stride, F f)
{
    const uint64_t size = items.size();
    for (uint64_t index = first; index < size; index += stride)
        f(items.at(index));
}

// One item of the TD update: a zero step touches nothing.  add as ntuple_update takes it.
template <uint32_t T, class Items, class Shape, class Add>
G2048_DEV void ntuple_item_update(const Items &items, const int64_t *delta, typename Items::Item it, uint32_t lr_shift, const Shape &sh,
                                  Add add)
{
    const int32_t step = ntuple_step(items.td_delta(delta, it), lr_shift);
    if (step != 0)
        ntuple_update<T>(items.packed(it), sh, step, add);
}

// One item of TC phase W: d == 0 touches nothing.  add as ntuple_tc_weights takes it.
template <uint32_t T, class Items, class Shape, class Add>
G2048_DEV void ntuple_item_tc_weights(const Items &items, const int64_t *delta, typename Items::Item it, uint32_t lr_shift,
                                      const Shape &sh, const int64_t *err, const int64_t *mag, Add add)
{
    const int64_t d = items.tc_delta(delta, it);
    if (d != 0)
        ntuple_tc_weights<T>(items.packed(it), sh, d, lr_shift, err, mag, add);
}

// One item of TC phase A, the same items as phase W.  add as ntuple_tc_accum takes it.
template <uint32_t T, class Items, class Shape, class Add>
G2048_DEV void ntuple_item_tc_accum(const Items &items, const int64_t *delta, typename Items::Item it, const Shape &sh, Add add)
{
    const int64_t d = items.tc_delta(delta, it);
    if (d != 0)
        ntuple_tc_accum<T>(items.packed(it), sh, d, add);
}

// Batch-mean update (g2048_ntuple_mean_update_plain / g2048_ntuple_mean_trace_update, include/g2048.h):
// every entry reached in a call moves ONCE, by the mean of the errors that reached it, where the updates above move it once
// per reach.  Two caller-owned arrays shaped like the weights, zero before and after every complete call: sum (int64, wraps
// mod 2^64) and count (uint32, wraps mod 2^32).  d = tc_delta of the item; d == 0 touches nothing in either phase.
//   phase SUM:    sum[j] += d;  count[j] += 1                                    for each of the item's 8T look-ups j
//   phase APPLY:  c = exchange(count[j], 0);  if c != 0:  a = exchange(sum[j], 0),
//                 weights[j] += ntuple_step(floor(a / c), lr_shift)              for the same items and look-ups
// Whichever reach of an entry comes first in APPLY owns it; all the others read c == 0 and do nothing.  sum and count are
// sums of integer adds and are complete before APPLY starts (a launch of its own), so the step does not depend on who the
// owner is: the same bits in any lane order.  An entry two symmetries of one board reach has both reaches in sum and count.

// floor(a / c) for c >= 1: C++ division truncates, so a negative a with a remainder is one too high
G2048_DEV int64_t ntuple_mean_floor_div(int64_t a, uint32_t c)
{
    const int64_t q = a / static_cast<int64_t>(c);
    return q - ((a % static_cast<int64_t>(c)) < 0 ? 1 : 0);
}

// Phase SUM of one board, d != 0: add(offset, d) for each of the 8T look-ups (sum += d, count += 1).
template <uint32_t T, class Shape, class Add> G2048_DEV void ntuple_mean_sum(uint64_t packed, const Shape &sh, int64_t d, Add add)
{
    const uint32_t base = ntuple_stage_base(packed, sh);
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s)
#pragma unroll
        for (uint32_t t = 0; t < T; ++t)
            add(ntuple_offset(packed, sh, s, t, base), d);
}

// Phase APPLY of one board: all 8T offsets, then all 8T claims c = claim(offset) (exchange(count, 0): independent, in flight
// together, as the loads of ntuple_tc_weights), then for every claim that is not 0 a = take(offset) (exchange(sum, 0)), the
// one 64-bit division of that entry, and add(offset, step) where the step is not 0.
template <uint32_t T, class Shape, class Claim, class Take, class Add>
G2048_DEV void ntuple_mean_apply(uint64_t packed, const Shape &sh, uint32_t lr_shift, Claim claim, Take take, Add add)
{
    uint32_t off[8u * T];
    uint32_t c[8u * T];
    const uint32_t base = ntuple_stage_base(packed, sh);
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s)
#pragma unroll
        for (uint32_t t = 0; t < T; ++t)
            off[s * T + t] = ntuple_offset(packed, sh, s, t, base);
#pragma unroll
    for (uint32_t j = 0; j < 8u * T; ++j)
        c[j] = claim(off[j]);
#pragma unroll
    for (uint32_t j = 0; j < 8u * T; ++j) {
        if (c[j] == 0)
            continue;
        const int32_t step = ntuple_step(ntuple_mean_floor_div(take(off[j]), c[j]), lr_shift);
        if (step != 0)
            add(off[j], step);
    }
}

// One item of phase SUM: d == 0 touches nothing.  add as ntuple_mean_sum takes it.
template <uint32_t T, class Items, class Shape, class Add>
G2048_DEV void ntuple_item_mean_sum(const Items &items, const int64_t *delta, typename Items::Item it, const Shape &sh, Add add)
{
    const int64_t d = items.tc_delta(delta, it);
    if (d != 0)
        ntuple_mean_sum<T>(items.packed(it), sh, d, add);
}

// One item of phase APPLY, the same items as phase SUM.  claim, take and add as ntuple_mean_apply takes them.
template <uint32_t T, class Items, class Shape, class Claim, class Take, class Add>
G2048_DEV void ntuple_item_mean_apply(const Items &items, const int64_t *delta, typename Items::Item it, uint32_t lr_shift,
                                      const Shape &sh, Claim claim, Take take, Add add)
{
    if (items.tc_delta(delta, it) != 0)
        ntuple_mean_apply<T>(items.packed(it), sh, lr_shift, claim, take, add);
}

// n-tuple delay (g2048_ntuple_delay_push / g2048_ntuple_delay_update / g2048_ntuple_tc_delay_update, include/g2048.h,
// INTEGRATION.md §19; the delayed TD(lambda) and TC(lambda) of Jaskowski 2017): the errors an afterstate earns over the H
// pushes after its own are collected in a per-board accumulator and applied to the tables ONCE, when the afterstate leaves
// the ring or its episode ends -- one board's worth of adds per board per step whatever H is, where a trace update issues up
// to H.  The delay ring is the trace ring plus accumulators, caller-owned, zero-initialised, one per engine or shard:
//   H, lam, hist, len   as for the traces
//   acc   int64 [H][n]  slot-major, 8-byte aligned: the error collected so far by the afterstate in that slot
// delay push(slot), for every board i (the caller advances slot by one mod H first, as for the trace push):
//   l = ntuple_trace_kept(len[i], H);   L = min(l + 1, H)
//   hist[slot][i], delta[i], len[i]     exactly as the trace push writes them
//   d = ntuple_tc_delta(delta[i])
//   acc[slot][i] = d                                                                    (k = 0: overwritten, never added to)
//   for k in 1..L-1:  acc[ntuple_trace_slot(slot, k, H)][i] += ntuple_trace_dk(d, ntuple_trace_decay(lam, k))
// |acc| <= 8 * 2^40 = 2^43.  Push is total for any len byte.  An accumulator is written by its board's lane only: no atomics.
// delay update(slot, mode), slot that of the last push, one work item per (k, i), k < L = min(len[i] & 0x7f, H),
// ended = len[i] & 0x80:
//   mode kNtupleDelayStep  (after every push):           the item is due iff  ended  or  k == H-1
//   mode kNtupleDelayFlush (once, when training stops):  the item is due iff  !ended and k != H-1
//   a due item:  D = ntuple_tc_delta(acc[ntuple_trace_slot(slot, k, H)][i]);   a = hist[the same slot][i]
//     TD:    step = ntuple_step(D, lr_shift);  ntuple_update(a, step);  a zero step touches nothing
//     TC W:  ntuple_tc_weights(a, D, ...), err and mag as before the call;   TC A:  ntuple_tc_accum(a, D);   D == 0 touches nothing
// The update writes nothing to the ring.  FLUSH is defined for the state right after a STEP update, and the caller zeroes len
// behind it; FLUSH twice, or FLUSH without the STEP update before it, applies errors twice or not at all.  Over any pushes
// with STEP updates and one FLUSH every pushed afterstate a_t is applied exactly once, with the total
// sum over k = 0..m of (clamp(delta_{t+k}) * p_k) >> 16, m ending at H-1, at the first push that terminated or at the last
// push.  The table updates are sums of integer adds from launches that read no entry they write (W and A stay separate
// launches): the same bits for any lane, wave, block, launch geometry or shard split.  H = 1 is the trace update at H = 1.
constexpr uint32_t kNtupleDelayStep = 0, kNtupleDelayFlush = 1; // = G2048_NTUPLE_DELAY_STEP, G2048_NTUPLE_DELAY_FLUSH (g2048.h)

// The accumulator pass of push for one board: L as push forms it (1..H), d = ntuple_tc_delta(delta), acc(plane) a reference to
// the board's accumulator in that plane.  The L-1 read-modify-writes are independent: all loads, then all stores.  p_k by at
// most kNtupleTraceMax - 1 multiplies.
template <class Acc> G2048_DEV void ntuple_delay_collect(uint32_t L, int64_t d, uint32_t lam, uint32_t slot, uint32_t H, Acc acc)
{
    int64_t old[kNtupleTraceMax - 1u];
#pragma unroll
    for (uint32_t k = 1; k < kNtupleTraceMax; ++k)
        if (k < L)
            old[k - 1u] = acc(ntuple_trace_slot(slot, k, H));
    uint64_t p = kNtupleTcOne;
#pragma unroll
    for (uint32_t k = 1; k < kNtupleTraceMax; ++k) {
        p = (p * lam) >> 16; // = ntuple_trace_decay(lam, k)
        if (k < L)
            acc(ntuple_trace_slot(slot, k, H)) = old[k - 1u] + ntuple_trace_dk(d, static_cast<uint32_t>(p));
    }
    acc(slot) = d;
}

// One board of the delay push, after its afterstate is stored: returns delta[i] and updates the len byte and the accumulators.
template <class Acc>
G2048_DEV int64_t ntuple_delay_push(uint8_t &len_i, int64_t best_next, int64_t after_value, bool terminated, uint32_t lam, uint32_t slot,
                                    uint32_t H, Acc acc)
{
    const uint32_t L = ntuple_trace_kept(len_i, H) + 1u; // <= H + 1; collect needs min(L, H)
    const int64_t delta = ntuple_trace_delta(best_next, after_value, terminated);
    len_i = static_cast<uint8_t>(ntuple_trace_push_len(len_i, H, terminated));
    ntuple_delay_collect(L < H ? L : H, ntuple_tc_delta(delta), lam, slot, H, acc);
    return delta;
}

// whether item (k, i) of a delay update has something to apply in this mode; len_i is its only load so far
G2048_DEV bool ntuple_delay_due(uint32_t len_i, uint32_t k, uint32_t H, uint32_t mode)
{
    if (k >= ntuple_trace_len(len_i, H))
        return false;
    const bool leaving = (len_i & kNtupleTraceEnded) != 0u || k + 1u == H;
    return leaving != (mode == kNtupleDelayFlush);
}

// The third item source: item k * n + i = the afterstate of board i that is k pushes old, as NtupleTraceItems, but what it
// applies is the accumulator of that slot and only when the item is due.  The accumulators arrive through the `delta`
// argument of the item operations -- acc, the base of plane 0 -- so the kernels keep one signature for the three sources
// (as a member the compiler's report is the same: profiles/r22_ntuple_delay_resource_usage.txt).  Item index, slot base of
// hist and plane base of acc are 64-bit.
struct NtupleDelayItems {
    const uint4 *hist;  // [H][n] boards
    const uint8_t *len; // [n]
    uint32_t n, H, slot, mode; // slot: that of the last push
    using Item = NtupleTraceItems::Item;
    G2048_MEMBER uint64_t size() const { return static_cast<uint64_t>(H) * n; }
    G2048_MEMBER Item at(uint64_t index) const
    {
        Item it;
        ntuple_trace_split(index, n, H, it.k, it.i);
        return it;
    }
    G2048_MEMBER int64_t td_delta(const int64_t *acc, Item it) const
    {
        if (!ntuple_delay_due(len[it.i], it.k, H, mode))
            return 0;
        return ntuple_tc_delta(acc[static_cast<uint64_t>(ntuple_trace_slot(slot, it.k, H)) * n + it.i]);
    }
    G2048_MEMBER int64_t tc_delta(const int64_t *acc, Item it) const { return td_delta(acc, it); }
    G2048_MEMBER uint64_t packed(Item it) const
    {
        return ntuple_pack(load_board(hist + static_cast<uint64_t>(ntuple_trace_slot(slot, it.k, H)) * n, it.i));
    }
};

// ------------------------------------------------------------------- n-tuple expectimax
// g2048_ntuple_search (include/g2048.h): the expectimax of above with the network at the leaves.
// Integers only, so every split of the tree across lanes gives the same bits.  With V, move(b, d) = (a_d, g_d, legal)
// as in the n-tuple block, a cell empty when it equals 0 and E(a) the number of empty cells:
//   A_0(a) = V(a)
//   S_k(b) = max over legal d of ((g_d << F) + A_k(a_d));   0 when no move is legal           (S_0 = evaluate's best)
//   A_k(a) = floor(sum over empty c of (9 S_{k-1}(a, 2 in c) + S_{k-1}(a, 4 in c)) / (10 E(a)))   for k >= 1
//   value[d] = (g_d << F) + A_D(a_d), kNtupleIllegal where d is illegal; action = the smallest d of largest value among
//   the legal d, 0 when none is legal.  D = 1..2 (kNtupleSearchMaxDepth).
// floor rounds toward minus infinity (weights are signed: the sum may be negative); an afterstate of a legal move has
// E >= 1.  Bounds: |V| <= 2^37 and g < 2^31, so |(g << F) + V| < 2^48 and every level adds at most one more g << F:
// |value| < 2^50.  A chance sum has weights that add up to 10 E <= 150: it stays below 150 * 2^50 < 2^58, an int64 in
// every lane, and the 2^60 bias of ntuple_key still makes every legal key positive.
constexpr uint32_t kNtupleSearchMaxDepth = 2; // = G2048_NTUPLE_SEARCH_MAX_DEPTH (g2048.h)

// floor(a / b) for b > 0: C++ '/' truncates toward zero, one too high for a negative inexact quotient
G2048_DEV int64_t floor_div(int64_t a, int64_t b)
{
    const int64_t q = a / b;
    return q - (a - q * b < 0 ? 1 : 0);
}

template <int D, uint32_t T, class Shape, class Tables>
G2048_DEV int64_t ntuple_search_state(const Board &b, const Shape &sh, uint32_t F, const int32_t *weights, const Tables &tb);

// Part of the chance-node sum of afterstate `a`: the items sub, sub + K, ... of chance_items, each weight * S_{D-1}.
template <int D, uint32_t T, class Shape, class Tables>
G2048_DEV int64_t ntuple_chance_partial(const Board &a, uint32_t sub, uint32_t K, const Shape &sh, uint32_t F,
                                        const int32_t *weights, const Tables &tb)
{
    int64_t sum = 0;
    chance_items(a, sub, K, [&](const Board &child, uint32_t weight) {
        sum += static_cast<int64_t>(weight) * ntuple_search_state<D - 1, T>(child, sh, F, weights, tb);
    });
    return sum;
}

// A_D(a); for D >= 1 a must have an empty cell
template <int D, uint32_t T, class Shape, class Tables>
G2048_DEV int64_t ntuple_after_value(const Board &a, const Shape &sh, uint32_t F, const int32_t *weights, const Tables &tb)
{
    if constexpr (D == 0)
        return ntuple_value<T>(ntuple_pack(a), sh, weights);
    else
        return floor_div(ntuple_chance_partial<D, T>(a, 0u, 1u, sh, F, weights, tb), 10 * static_cast<int64_t>(count_empty(a)));
}

// S_D(b).  As in search_value the four moves are one loop body with a run-time selector row and the depths D .. 0 one
// inlined body each: no recursion and no per-lane array at run time.  A leaf (D = 0) looks up its moves one after the
// other, 8T gathers in flight at a time, which keeps the registers of T = 8 out of scratch.
template <int D, uint32_t T, class Shape, class Tables>
G2048_DEV int64_t ntuple_search_state(const Board &b, const Shape &sh, uint32_t F, const int32_t *weights, const Tables &tb)
{
    int64_t best = 0;
    bool any = false;
#pragma unroll 1
    for (uint32_t m = 0; m < 4u; ++m) {
        Board a = b;
        uint32_t gain;
        if (move_sel(a, tb.move_sel(m), gain)) {
            const int64_t q = static_cast<int64_t>(static_cast<uint64_t>(gain) << F) + ntuple_after_value<D, T>(a, sh, F, weights, tb);
            best = !any || q > best ? q : best;
            any = true;
        }
    }
    return best;
}

// The root on one thread: value[4] and the action.  The kernel splits the same chance sums across lanes
// (ntuple_chance_partial) and joins the four keys with shuffles.
template <int D, uint32_t T, class Shape, class Tables>
G2048_DEV uint32_t ntuple_search_root(const Board &cells, const Shape &sh, uint32_t F, const int32_t *weights,
                                      const Tables &tb, int64_t value[4])
{
    uint64_t best = 0;
    for (uint32_t d = 0; d < 4u; ++d) {
        Board a = cells;
        uint32_t gain;
        const bool legal = move_sel(a, tb.move_sel(d), gain);
        value[d] = legal ? static_cast<int64_t>(static_cast<uint64_t>(gain) << F) + ntuple_after_value<D, T>(a, sh, F, weights, tb)
                         : kNtupleIllegal;
        const uint64_t key = ntuple_key(value[d], legal, d);
        best = key > best ? key : best;
    }
    return root_key_action(best);
}

// ------------------------------------------------------------------- n-tuple deep search
// g2048_ntuple_deep_search (include/g2048.h): the definition of above at D = 2..3, split so that a whole
// workgroup works on ONE board.  Bounds at D = 3, re-derived: a leaf is |V| <= 8 * 8 * 2^31 = 2^37; S_0 adds one gain << F with
// gain < 2^31 and F <= 16, below 2^47; every level above adds one more, and floor() of a weighted mean does not leave the range
// of its terms: |value| <= 2^37 + 4 * 2^47 < 2^50 with the root's own gain.  The weights of a chance node add up to
// 10 E <= 150: any partial sum of it, in any order, stays below 150 * 2^50 < 2^58 -- an int64, and value + 2^60 of ntuple_key
// is still positive.  (Depth 2 has one gain less.)
//
// The tree has a floor() at every chance node, so it is no flat sum: it is reduced in two levels over a table that the
// kernel keeps in LDS and the host check in a plain struct (NtupleDeepLds).  P lanes, lane = 0 .. P-1, run the steps below with
// a barrier after each; every step is a function here, so the host runs the kernel's split with any P:
//   root     lanes 0..3: the root afterstate of direction d1, its gain and its 2 E chance items (0: illegal or masked out)
//   expand   entry e = 4 * item1 + d2 for the level-1 items item1 = (d1, cell, tile) in direction order, at most 4 * 30:
//            the afterstate of move d2 on the item's child board, its gain, and its count of work units: its 2 E chance
//            items, 0 where d2 is illegal
//   scan     prefix sums of the counts: unit u belongs to the entry e with first[e] <= u < first[e + 1]
//   leaves   unit u = lane, lane + P, ...: acc[e] += weight * S_{D-2}(child of the unit) -- a unit is a depth-1 tree at
//            D = 3 and the four look-ups of evaluate at D = 2, the straight-line code of ntuple_search_state; integer adds commute
//   fold     item1 = lane, lane + P, ...: S_{D-1}(child) = max over legal d2 of (gain << F) + floor(acc / 10 E), 0 when no
//            d2 is legal; sum[d1] += weight * S_{D-1}
//   finish   lane 0: value[d1] = (gain << F) + floor(sum[d1] / 10 E), the keys and the action
constexpr uint32_t kNtupleDeepMinDepth = 2, kNtupleDeepMaxDepth = 3; // = G2048_NTUPLE_DEEP_MIN/MAX_DEPTH (g2048.h)
constexpr uint32_t kNtupleDeepMaxItems = 4u * 30u;                  // level-1 items: a root afterstate has at most 15 empty cells
constexpr uint32_t kNtupleDeepMaxEntries = 4u * kNtupleDeepMaxItems;

struct NtupleDeepLds {
    Board after[kNtupleDeepMaxEntries];     // afterstate of entry e
    long long acc[kNtupleDeepMaxEntries];   // its chance sum
    uint32_t gain[kNtupleDeepMaxEntries];
    uint32_t first[kNtupleDeepMaxEntries + 1u]; // first work unit of entry e; [4 * items] = the number of units
    uint32_t count[kNtupleDeepMaxItems];    // byte d2 = the units of entry 4 * item1 + d2 (<= 30)
    Board root_after[4];
    long long root_sum[4];
    uint32_t root_gain[4], root_items[4];   // 2 E of the root afterstate; 0 = illegal
};

// Chance item t of afterstate `a` (the order of chance_items): the child board and its weight
G2048_DEV Board ntuple_deep_item(const Board &a, uint32_t t, uint32_t &weight)
{
    uint32_t m = empty_bits(a);
#pragma unroll 1
    for (uint32_t k = 0; k < (t >> 1); ++k)
        m &= m - 1u;
    const uint32_t v = 1u + (t & 1u);
    weight = v == 1u ? 9u : 1u;
    return place(a, g2048_ctz(m), v);
}

// Where level-1 item t sits: its root direction and its item index there.  t < the sum of root_items.
G2048_DEV void ntuple_deep_item1(const NtupleDeepLds &l, uint32_t t, uint32_t &d1, uint32_t &local)
{
    d1 = 0;
    local = t;
#pragma unroll
    for (uint32_t d = 0; d < 3u; ++d) {
        const bool past = d1 == d && local >= l.root_items[d];
        local -= past ? l.root_items[d] : 0u;
        d1 += past ? 1u : 0u;
    }
}
G2048_DEV uint32_t ntuple_deep_items(const NtupleDeepLds &l)
{
    return l.root_items[0] + l.root_items[1] + l.root_items[2] + l.root_items[3];
}

// root: lanes 0..3 (the others return).  active = false: a masked-out board has no legal direction.
template <class Tables>
G2048_DEV void ntuple_deep_root(NtupleDeepLds &l, const Board &cells, bool active, uint32_t lane, const Tables &tb)
{
    if (lane >= 4u)
        return;
    Board a = cells;
    uint32_t gain;
    const bool legal = move_sel(a, tb.move_sel(lane), gain) && active;
    l.root_after[lane] = a;
    l.root_gain[lane] = gain;
    l.root_items[lane] = legal ? 2u * count_empty(a) : 0u;
    l.root_sum[lane] = 0;
}

template <class Tables> G2048_DEV void ntuple_deep_expand(NtupleDeepLds &l, uint32_t lane, uint32_t P, const Tables &tb)
{
    const uint32_t entries = 4u * ntuple_deep_items(l);
#pragma unroll 1
    for (uint32_t e = lane; e < entries; e += P) {
        uint32_t d1, local, weight, gain;
        ntuple_deep_item1(l, e >> 2, d1, local);
        Board a = ntuple_deep_item(l.root_after[d1], local, weight);
        const bool legal = move_sel(a, tb.move_sel(e & 3u), gain);
        l.after[e] = a;
        l.gain[e] = gain;
        l.acc[e] = 0;
        reinterpret_cast<uint8_t *>(l.count)[e] = static_cast<uint8_t>(legal ? 2u * count_empty(a) : 0u);
    }
}

G2048_DEV uint32_t ntuple_deep_byte_sum(uint32_t w) { return (w * 0x01010101u) >> 24; } // four bytes, each <= 30

G2048_DEV void ntuple_deep_scan(NtupleDeepLds &l, uint32_t lane, uint32_t P)
{
    const uint32_t items = ntuple_deep_items(l);
    if (lane == 0u)
        l.first[0] = 0u;
#pragma unroll 1
    for (uint32_t t = lane; t < items; t += P) {
        uint32_t at = 0;
#pragma unroll 1
        for (uint32_t u = 0; u < t; ++u)
            at += ntuple_deep_byte_sum(l.count[u]);
        uint32_t w = l.count[t];
#pragma unroll
        for (uint32_t d2 = 0; d2 < 4u; ++d2, w >>= 8) {
            at += w & 0xffu;
            l.first[4u * t + d2 + 1u] = at;
        }
    }
}

// the entry of work unit u < first[entries]: the last e with first[e] <= u (an entry without units is never the answer)
G2048_DEV uint32_t ntuple_deep_entry(const NtupleDeepLds &l, uint32_t entries, uint32_t u)
{
    uint32_t lo = 0, hi = entries; // first[lo] <= u < first[hi]
#pragma unroll 1
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        const bool left = l.first[mid] > u;
        hi = left ? mid : hi;
        lo = left ? lo : mid;
    }
    return lo;
}

// add(e, x): acc[e] += x, atomically among the lanes
template <int D, uint32_t T, class Shape, class Tables, class Add>
G2048_DEV void ntuple_deep_leaves(const NtupleDeepLds &l, uint32_t lane, uint32_t P, const Shape &sh, uint32_t F, const int32_t *weights,
                                  const Tables &tb, Add add)
{
    static_assert(D >= 2 && D <= 4, "kNtupleDeepMinDepth .. kNtupleDeepMaxDepth, and kNtupleAdaptiveMaxDepth (n-tuple adaptive search)");
    const uint32_t entries = 4u * ntuple_deep_items(l), units = l.first[entries];
#pragma unroll 1
    for (uint32_t u = lane; u < units; u += P) {
        const uint32_t e = ntuple_deep_entry(l, entries, u);
        uint32_t weight;
        const Board child = ntuple_deep_item(l.after[e], u - l.first[e], weight);
        add(e, static_cast<int64_t>(weight) * ntuple_search_state<D - 2, T>(child, sh, F, weights, tb));
    }
}

// add(d1, x): root_sum[d1] += x, atomically among the lanes
template <class Add> G2048_DEV void ntuple_deep_fold(const NtupleDeepLds &l, uint32_t lane, uint32_t P, uint32_t F, Add add)
{
    const uint32_t items = ntuple_deep_items(l);
#pragma unroll 1
    for (uint32_t t = lane; t < items; t += P) {
        int64_t best = 0;
        bool any = false;
        uint32_t w = l.count[t];
#pragma unroll 1
        for (uint32_t d2 = 0; d2 < 4u; ++d2, w >>= 8) {
            const uint32_t e = 4u * t + d2, units = w & 0xffu;
            if (units == 0u)
                continue;
            const int64_t q = static_cast<int64_t>(static_cast<uint64_t>(l.gain[e]) << F) + floor_div(l.acc[e], 5 * static_cast<int64_t>(units));
            best = !any || q > best ? q : best;
            any = true;
        }
        uint32_t d1, local;
        ntuple_deep_item1(l, t, d1, local);
        add(d1, ((local & 1u) ? 1 : 9) * best);
    }
}

// finish: one lane.  value[4] and the action, as ntuple_search_root gives them.
G2048_DEV uint32_t ntuple_deep_finish(const NtupleDeepLds &l, uint32_t F, int64_t value[4])
{
    uint64_t best = 0;
    for (uint32_t d = 0; d < 4u; ++d) {
        const bool legal = l.root_items[d] != 0u;
        value[d] = legal ? static_cast<int64_t>(static_cast<uint64_t>(l.root_gain[d]) << F) +
                               floor_div(l.root_sum[d], 5 * static_cast<int64_t>(l.root_items[d]))
                         : kNtupleIllegal;
        const uint64_t key = ntuple_key(value[d], legal, d);
        best = key > best ? key : best;
    }
    return root_key_action(best);
}

// ------------------------------------------------------------------- n-tuple adaptive search
// g2048_ntuple_adaptive_search (include/g2048.h): the definition of "n-tuple expectimax" at a depth per
// board, D = schedule[E0(b)] in 0..4 with E0 the board's own empty cells.  The table and the steps are those of the deep
// search above with a run-time D, the same for every lane that works on the board:
//   D = 0     root, where lane d also looks up V(a_d) into root_sum[d]; finish adds the gain and divides nothing (evaluate's q)
//   D = 1     root; leaves1: unit = level-1 item = lane, lane + P, ...: root_sum[d1] += weight * S_0(child); finish
//   D = 2..4  root, expand, scan, leaves, fold, finish with a unit = S_{D-2} of a level-2 item: at D = 4 the depth-2 tree of
//             ntuple_search_state<2> on one lane
// Bounds at D = 4: |V| <= 2^37, S_0 adds one gain << F < 2^47 and S_1, S_2, S_3 and the root one more each, floor() of a
// weighted mean stays within its terms: |value| <= 2^37 + 5 * 2^47 < 2^50.  A chance node's weights add up to 10 E <= 150: a
// partial sum, in any order, stays below 150 * 2^50 < 2^58, and value + 2^60 of ntuple_key is positive.
constexpr uint32_t kNtupleAdaptiveMaxDepth = 4;   // = G2048_NTUPLE_ADAPTIVE_MAX_DEPTH (g2048.h)
constexpr uint32_t kNtupleAdaptiveSkipped = 0xffu; // = G2048_NTUPLE_ADAPTIVE_SKIPPED

// schedule[17] as a kernel argument that no lane indexes in memory: nibble E of lo = schedule[E] for E < 16, hi = schedule[16]
struct NtupleAdaptiveSchedule {
    uint64_t lo;
    uint32_t hi;
};
G2048_HOST_DEV NtupleAdaptiveSchedule ntuple_adaptive_schedule(const uint8_t schedule[17])
{
    NtupleAdaptiveSchedule s{0u, schedule[16]};
    for (uint32_t e = 0; e < 16u; ++e)
        s.lo |= static_cast<uint64_t>(schedule[e] & 0xfu) << (4u * e);
    return s;
}
G2048_DEV uint32_t ntuple_adaptive_depth(const NtupleAdaptiveSchedule &s, const Board &cells)
{
    const uint32_t e0 = count_empty(cells);
    return e0 < 16u ? static_cast<uint32_t>(s.lo >> (4u * e0)) & 0xfu : s.hi;
}

// root: ntuple_deep_root, and at depth 0 lane d looks up V of its afterstate (a depth above 0 starts its sums at 0)
template <uint32_t T, class Shape, class Tables>
G2048_DEV void ntuple_adaptive_root(NtupleDeepLds &l, const Board &cells, bool active, uint32_t depth, uint32_t lane, const Shape &sh,
                                    const int32_t *weights, const Tables &tb)
{
    ntuple_deep_root(l, cells, active, lane, tb);
    if (depth == 0u && lane < 4u && l.root_items[lane] != 0u)
        l.root_sum[lane] = ntuple_value<T>(ntuple_pack(l.root_after[lane]), sh, weights);
}

// leaves of depth 1: add(d1, x): root_sum[d1] += x, atomically among the lanes
template <uint32_t T, class Shape, class Tables, class Add>
G2048_DEV void ntuple_adaptive_leaves1(const NtupleDeepLds &l, uint32_t lane, uint32_t P, const Shape &sh, uint32_t F,
                                       const int32_t *weights, const Tables &tb, Add add)
{
    const uint32_t items = ntuple_deep_items(l);
#pragma unroll 1
    for (uint32_t t = lane; t < items; t += P) {
        uint32_t d1, local, weight;
        ntuple_deep_item1(l, t, d1, local);
        const Board child = ntuple_deep_item(l.root_after[d1], local, weight);
        add(d1, static_cast<int64_t>(weight) * ntuple_search_state<0, T>(child, sh, F, weights, tb));
    }
}

// leaves of depth 2..4: ntuple_deep_leaves at the board's depth.  The branch is the same for every lane of the board.
template <uint32_t T, class Shape, class Tables, class Add>
G2048_DEV void ntuple_adaptive_leaves(const NtupleDeepLds &l, uint32_t depth, uint32_t lane, uint32_t P, const Shape &sh, uint32_t F,
                                      const int32_t *weights, const Tables &tb, Add add)
{
    if (depth == 2u)
        ntuple_deep_leaves<2, T>(l, lane, P, sh, F, weights, tb, add);
    else if (depth == 3u)
        ntuple_deep_leaves<3, T>(l, lane, P, sh, F, weights, tb, add);
    else
        ntuple_deep_leaves<4, T>(l, lane, P, sh, F, weights, tb, add);
}

// finish: one lane.  Depth 0 has V itself in root_sum, every other depth a chance sum to divide (ntuple_deep_finish).
G2048_DEV uint32_t ntuple_adaptive_finish(const NtupleDeepLds &l, uint32_t depth, uint32_t F, int64_t value[4])
{
    if (depth != 0u)
        return ntuple_deep_finish(l, F, value);
    uint64_t best = 0;
    for (uint32_t d = 0; d < 4u; ++d) {
        const bool legal = l.root_items[d] != 0u;
        value[d] = legal ? static_cast<int64_t>(static_cast<uint64_t>(l.root_gain[d]) << F) + l.root_sum[d] : kNtupleIllegal;
        const uint64_t key = ntuple_key(value[d], legal, d);
        best = key > best ? key : best;
    }
    return root_key_action(best);
}

// ------------------------------------------------------------------- n-tuple reduced search
// g2048_ntuple_reduced_search (include/g2048.h): the adaptive search of above with the rare branches
// searched shallower.  A child board made by a 4 spawn is searched R = reduce4 (1..2) plies shallower than its 2 sibling:
//   A^R_0(a) = V(a)
//   S^R_k(b) = max over legal d of ((g_d << F) + A^R_k(a_d));   0 when no move is legal
//   A^R_k(a) = floor(sum over empty c of (9 S^R_{k-1}(a, 2 in c) + S^R_{max(k-1-R, 0)}(a, 4 in c)) / (10 E(a)))   for k >= 1
//   value[d] = (g_d << F) + A^R_D(a_d), D = schedule[E0(b)] in 0..4; kNtupleIllegal, the action and the mask as above.
// The rule is integer and path-local: no probability and no threshold, so the bits do not depend on the split.  S^R_0 = S_0 and
// S^R_1 = S_1 for both R (the children of S_1 are leaves already); D = 0 and D = 1 are the adaptive search.  Bounds: every term
// is one the adaptive block bounds -- a tree here is a tree there with some levels left out -- so |value| < 2^50, a partial
// sum of a chance node stays below 150 * 2^50 < 2^58, and value + 2^60 of ntuple_key is positive.
//
// The table and the steps are those of the deep search; what differs at D = 2..4:
//   r1    the remaining depth of a level-1 item with tile v1: max(D - 1 - R [v1 is 4], 0), in 0..3
//   r2    the remaining depth of a unit, a level-2 item with tile v2 under an item of r1 >= 1: max(r1 - 1 - R [v2 is 4], 0), 0..2
//   expand   as ntuple_deep_expand, but an entry of an item with r1 = 0 is a LEAF ENTRY: its count is 1 where d2 is legal.  An
//            entry with a chance node has 2 E >= 2 units, always even, so the count byte holds the three states by itself:
//            0 illegal, 1 leaf entry, 2 E chance node.  No flag is stored anywhere else.
//   scan     ntuple_deep_scan, unchanged (a count is still <= 30)
//   leaves   a unit of a leaf entry: acc[e] += V(after[e]); any other unit: acc[e] += weight * S^R_{r2}(child), the tree of
//            ntuple_reduced_state on the lane.  Units of one wave differ by up to two plies; they run ONE loop nest with run-time
//            depths (below), so lanes of unequal depth share its instructions where their trip counts overlap.
//   fold     S^R_{r1}(child) = max over legal d2 of (gain << F) + (count 1: acc, no division; else floor(acc / 10 E))
//   D = 0, D = 1, root, finish: the adaptive steps, unchanged.
constexpr uint32_t kNtupleReduce4Min = 1, kNtupleReduce4Max = 2; // = G2048_NTUPLE_REDUCE4_MIN/MAX (g2048.h)

G2048_DEV uint32_t ntuple_reduced_below(uint32_t r, uint32_t R, bool four) // max(r - 1 - R [four], 0) for r >= 1
{
    const uint32_t less = 1u + (four ? R : 0u);
    return r > less ? r - less : 0u;
}
// r1 of level-1 item `local` of a root afterstate (odd = the 4 tile), D >= 1
G2048_DEV uint32_t ntuple_reduced_r1(uint32_t depth, uint32_t R, uint32_t local) { return ntuple_reduced_below(depth, R, (local & 1u) != 0u); }

// S^R_k(b) for a run-time k in 0..1, where it is S_k: every child of the chance node is a leaf.  One loop body for both k.
template <uint32_t T, class Shape, class Tables>
G2048_DEV int64_t ntuple_reduced_state1(const Board &b, uint32_t k, const Shape &sh, uint32_t F, const int32_t *weights, const Tables &tb)
{
    int64_t best = 0;
    bool any = false;
#pragma unroll 1
    for (uint32_t m = 0; m < 4u; ++m) {
        Board a = b;
        uint32_t gain;
        if (move_sel(a, tb.move_sel(m), gain)) {
            int64_t v;
            if (k == 0u) {
                v = ntuple_value<T>(ntuple_pack(a), sh, weights);
            } else {
                int64_t sum = 0;
                chance_items(a, 0u, 1u, [&](const Board &child, uint32_t weight) {
                    sum += static_cast<int64_t>(weight) * ntuple_search_state<0, T>(child, sh, F, weights, tb);
                });
                v = floor_div(sum, 10 * static_cast<int64_t>(count_empty(a)));
            }
            const int64_t q = static_cast<int64_t>(static_cast<uint64_t>(gain) << F) + v;
            best = !any || q > best ? q : best;
            any = true;
        }
    }
    return best;
}

// S^R_k(b) for a run-time k in 0..2: the tree of a work unit on one lane.  At k = 2 the 2 children of the chance node are S_1
// and the 4 children S_0, for both R (max(1 - R, 0) = 0); at k = 1 both are S_0.  No recursion and no per-lane array.
template <uint32_t T, class Shape, class Tables>
G2048_DEV int64_t ntuple_reduced_state(const Board &b, uint32_t k, const Shape &sh, uint32_t F, const int32_t *weights, const Tables &tb)
{
    int64_t best = 0;
    bool any = false;
#pragma unroll 1
    for (uint32_t m = 0; m < 4u; ++m) {
        Board a = b;
        uint32_t gain;
        if (move_sel(a, tb.move_sel(m), gain)) {
            int64_t v;
            if (k == 0u) {
                v = ntuple_value<T>(ntuple_pack(a), sh, weights);
            } else {
                int64_t sum = 0;
                chance_items(a, 0u, 1u, [&](const Board &child, uint32_t weight) {
                    const uint32_t below = k == 2u && weight == 9u ? 1u : 0u;
                    sum += static_cast<int64_t>(weight) * ntuple_reduced_state1<T>(child, below, sh, F, weights, tb);
                });
                v = floor_div(sum, 10 * static_cast<int64_t>(count_empty(a)));
            }
            const int64_t q = static_cast<int64_t>(static_cast<uint64_t>(gain) << F) + v;
            best = !any || q > best ? q : best;
            any = true;
        }
    }
    return best;
}

// expand at depth 2..4: ntuple_deep_expand with the leaf entries of the items whose r1 is 0
template <class Tables>
G2048_DEV void ntuple_reduced_expand(NtupleDeepLds &l, uint32_t depth, uint32_t R, uint32_t lane, uint32_t P, const Tables &tb)
{
    const uint32_t entries = 4u * ntuple_deep_items(l);
#pragma unroll 1
    for (uint32_t e = lane; e < entries; e += P) {
        uint32_t d1, local, weight, gain;
        ntuple_deep_item1(l, e >> 2, d1, local);
        Board a = ntuple_deep_item(l.root_after[d1], local, weight);
        const bool legal = move_sel(a, tb.move_sel(e & 3u), gain);
        const uint32_t units = ntuple_reduced_r1(depth, R, local) == 0u ? 1u : 2u * count_empty(a);
        l.after[e] = a;
        l.gain[e] = gain;
        l.acc[e] = 0;
        reinterpret_cast<uint8_t *>(l.count)[e] = static_cast<uint8_t>(legal ? units : 0u);
    }
}

// leaves at depth 2..4.  add(e, x): acc[e] += x, atomically among the lanes
template <uint32_t T, class Shape, class Tables, class Add>
G2048_DEV void ntuple_reduced_leaves(const NtupleDeepLds &l, uint32_t depth, uint32_t R, uint32_t lane, uint32_t P, const Shape &sh,
                                     uint32_t F, const int32_t *weights, const Tables &tb, Add add)
{
    const uint32_t entries = 4u * ntuple_deep_items(l), units = l.first[entries];
#pragma unroll 1
    for (uint32_t u = lane; u < units; u += P) {
        const uint32_t e = ntuple_deep_entry(l, entries, u);
        uint32_t d1, local;
        ntuple_deep_item1(l, e >> 2, d1, local);
        const uint32_t r1 = ntuple_reduced_r1(depth, R, local);
        if (r1 == 0u) { // a leaf entry: its one unit is V of the entry's afterstate
            add(e, ntuple_value<T>(ntuple_pack(l.after[e]), sh, weights));
            continue;
        }
        uint32_t weight;
        const Board child = ntuple_deep_item(l.after[e], u - l.first[e], weight);
        const uint32_t r2 = ntuple_reduced_below(r1, R, weight == 1u);
        add(e, static_cast<int64_t>(weight) * ntuple_reduced_state<T>(child, r2, sh, F, weights, tb));
    }
}

// fold at depth 2..4: ntuple_deep_fold, where an entry of count 1 is a leaf entry and divides nothing
template <class Add> G2048_DEV void ntuple_reduced_fold(const NtupleDeepLds &l, uint32_t lane, uint32_t P, uint32_t F, Add add)
{
    const uint32_t items = ntuple_deep_items(l);
#pragma unroll 1
    for (uint32_t t = lane; t < items; t += P) {
        int64_t best = 0;
        bool any = false;
        uint32_t w = l.count[t];
#pragma unroll 1
        for (uint32_t d2 = 0; d2 < 4u; ++d2, w >>= 8) {
            const uint32_t e = 4u * t + d2, units = w & 0xffu;
            if (units == 0u)
                continue;
            const int64_t chance = units == 1u ? l.acc[e] : floor_div(l.acc[e], 5 * static_cast<int64_t>(units));
            const int64_t q = static_cast<int64_t>(static_cast<uint64_t>(l.gain[e]) << F) + chance;
            best = !any || q > best ? q : best;
            any = true;
        }
        uint32_t d1, local;
        ntuple_deep_item1(l, t, d1, local);
        add(d1, ((local & 1u) ? 1 : 9) * best);
    }
}

// ------------------------------------------------------------------- carousel shaping
// Stage-balanced restarts for training a staged network (g2048_carousel_step, include/g2048.h, INTEGRATION.md §14;
// Jaskowski 2017): every episode starts from an empty board, so the weight sets of the late stages see a vanishing share of
// the updates.  The carousel remembers, per stage, the boards on which recent episodes ENTERED that stage, and starts new
// episodes from them, cycling over the stages.  Notation of the staged block: stage(b) from thr[0..S-2], cell = byte & 0x1f
// of an engine record.  State for n boards:
//   pool      uint8 [S][C][16]  ring of C records per stage, copied verbatim (cells and packed score); row 0 is never used
//   count     uint64 [S]        entries ever made into each stage
//   seen      uint8 [n]         highest stage this episode has been in; 0xff = not yet known
//   episodes  uint32 [n]        episodes this board has ended; wraps
// One operation, carousel_step, after a step with auto-reset on; g = index_offset + i.  With pool / count AS THEY WERE BEFORE
// THE CALL, for every board i:
//   terminated[i] != 0 (the record is already the fresh auto-reset board):
//       e = episodes[i];  episodes[i] = e + 1
//       M = the largest k with count[k] > 0, else 0;   k = (g + e) mod (M + 1)           (the sum in 64 bits)
//       k > 0 and count[k] > 0:   fill = min(count[k], C)
//                                 w = Philox4x32-10(ctr = (e, g, k, 0), key = (seed_lo, seed_hi ^ kCarouselKeyTag))[0]
//                                 j = (w * fill) >> 32;   record[i] = pool[k][j];   seen[i] = k
//       otherwise:                the fresh board stays;  seen[i] = stage(record[i])
//   terminated[i] == 0:  st = stage(record[i])
//       seen[i] == 0xff:  seen[i] = st, nothing is recorded
//       st > seen[i]:     board i is an ENTRY into stage st;  seen[i] = st
//       otherwise nothing happens  (stage(b) is not monotone over a game: seen is a maximum, not the last stage)
// Then the entries are recorded in ascending board index: of the m_k entries into stage k in this call, the one of rank r
// (0-based among them) is stored at pool[k][(count[k] + r) mod C] when r >= m_k - C, and dropped otherwise; then
// count[k] += m_k.  This is exactly the sequential loop over i = 0..n-1: the slots 0..min(count, C)-1 are the filled ones,
// so j is a physical slot; no two surviving entries share a slot.  Nothing about lanes, waves or workgroups enters the
// result: the rank is an ordered, batch-wide prefix count, not the arrival order at an atomic counter.
// seen holds 0..S-1 or 0xff between calls.  (Inside a call the per-board pass marks an entry by setting bit 7 of seen, and
// the scatter pass clears it: the mark is how the scatter pass finds the entries without reading the records again.)
constexpr uint32_t kCarouselKeyTag = 0x43524F55u; // "CROU": separates the restart stream from the spawn stream (no tag) and
                                                  // the Monte-Carlo stream (kMcKeyTag) under an equal seed
constexpr uint32_t kCarouselMinStages = 2, kCarouselMaxCapacity = 65536; // = G2048_CAROUSEL_MAX_CAPACITY (g2048.h)
constexpr uint32_t kCarouselUnknown = 0xffu, kCarouselEntryBit = 0x80u;

// The thresholds alone, as NtupleStagedShape::thr holds them: the carousel reads no table, and a staged shape would bring its
// 64 cell lists along as kernel arguments.
struct CarouselStages {
    uint32_t thr[kNtupleMaxStages - 1]; // thr[j], j < S - 1; kNtupleNoStage from there on
};

G2048_HOST_DEV CarouselStages carousel_stages(uint32_t n_stages, const uint16_t *thresholds)
{
    CarouselStages cs{};
    for (uint32_t j = 0; j < kNtupleMaxStages - 1u; ++j)
        cs.thr[j] = j + 1u < n_stages ? thresholds[j] : kNtupleNoStage;
    return cs;
}

// stage(b) of an engine record (or of plain cells): ntuple_stage on the carousel's own thresholds
G2048_DEV uint32_t carousel_stage(const Board &rec, const CarouselStages &cs)
{
    const uint32_t mask = ntuple_stage_mask(ntuple_pack(rec));
    uint32_t stage = 0;
    for (uint32_t j = 0; j < kNtupleMaxStages - 1u; ++j)
        stage += mask >= cs.thr[j] ? 1u : 0u;
    return stage;
}

// M: the largest k < S with count[k] > 0, else 0
G2048_HOST_DEV uint32_t carousel_top_stage(const uint64_t *count, uint32_t n_stages)
{
    uint32_t top = 0;
    for (uint32_t k = 1; k < n_stages; ++k)
        top = count[k] > 0 ? k : top;
    return top;
}

// k = (g + e) mod (M + 1) with the sum in 64 bits, formed from the two residues: M + 1 <= 8, nothing overflows
G2048_HOST_DEV uint32_t carousel_stage_choice(uint32_t g, uint32_t e, uint32_t top)
{
    const uint32_t m = top + 1u;
    return (g % m + e % m) % m;
}

// fill = min(count, C): the filled slots of a ring are 0..fill-1
G2048_HOST_DEV uint32_t carousel_fill(uint64_t count, uint32_t capacity)
{
    return count < capacity ? static_cast<uint32_t>(count) : capacity;
}

// j, the slot a restart of (episode e, global board g) into stage k reads: uniform over 0..fill-1, fill >= 1
G2048_DEV uint32_t carousel_sample(uint32_t e, uint32_t g, uint32_t k, uint32_t fill, uint32_t seed_lo, uint32_t seed_hi)
{
    return g2048_mulhi(philox4x32_10(e, g, k, 0u, seed_lo, seed_hi ^ kCarouselKeyTag).w[0], fill);
}

// The seen transition of a board whose episode goes on: the new seen byte, with kCarouselEntryBit set when the board is an
// entry into stage st (the scatter pass clears the bit).  A byte that is neither 0xff nor below st is left as it is.
G2048_HOST_DEV uint32_t carousel_seen_next(uint32_t seen, uint32_t st)
{
    if (seen == kCarouselUnknown)
        return st;
    return st > seen ? st | kCarouselEntryBit : seen;
}

// an entry mark left by carousel_seen_next
G2048_HOST_DEV bool carousel_is_entry(uint32_t seen) { return (seen & kCarouselEntryBit) != 0u && seen != kCarouselUnknown; }

// Does the entry of rank r among the m of its stage in this call survive (r >= m - C)?  r < m < 2^32.
G2048_HOST_DEV bool carousel_survives(uint32_t r, uint32_t m, uint32_t capacity) { return static_cast<uint64_t>(r) + capacity >= m; }

// count mod C, once per stage and call, so that the slot of an entry is 32-bit arithmetic
G2048_HOST_DEV uint32_t carousel_count_mod(uint64_t count, uint32_t capacity) { return static_cast<uint32_t>(count % capacity); }

// (count + r) mod C from count_mod = count mod C: both terms are below C <= 65536
G2048_HOST_DEV uint32_t carousel_slot(uint32_t count_mod, uint32_t r, uint32_t capacity) { return (count_mod + r % capacity) % capacity; }

// The workgroup ranges of the carousel kernels: workgroup w takes the boards [w * per, min(n, (w + 1) * per)), `per` a
// multiple of `block` lanes, and there are at most `cap` workgroups -- contiguous ranges, so that the index order of the
// entries is the order of (workgroup, chunk, wave, lane).
G2048_HOST_DEV uint64_t carousel_range(uint64_t n, uint32_t block, uint32_t cap)
{
    const uint64_t blocks = (n + block - 1u) / block;
    const uint64_t groups = blocks < cap ? blocks : cap;
    return (blocks + groups - 1u) / groups * block; // n >= 1
}

// ------------------------------------------------------------------- the 16-byte board RECORD
// What the engine keeps per board in HBM is ONE 16-byte record: bits [4:0] of byte j = exponent of
// cell j (0..31), and the 24-bit SCORE DEFICIT d in the three spare bits [7:5] of bytes 8..15
// (registers r[2], r[3]; bit k of d lives in bit 5 + k % 3 of byte 8 + k / 3).
//   d = (potential(board) - score) mod 2^24,   potential = sum over tiles of (e - 1) * 2^e.
// Why a deficit and not the score: a merge of two 2^e tiles raises the potential by exactly the 2^(e+1)
// it scores (game2048_env.py:253-254), a spawned 2 leaves it alone and a spawned 4 raises it by 4
// without scoring -- so d changes only when a 4 is spawned (d += 4), which in the spread layout is one
// carry-propagating add; the episodic score self.score (game2048_env.py:46,86,105) is recovered as
// potential - d where it is needed (episode end, get_scores).  No separate score array: a step reads
// and writes exactly the 16-byte record.  Scores are exact below 2^24 = 16 777 216 (the largest score
// a 4x4 game can reach is about 3.9 million).
constexpr uint32_t kCellBits = 0x1f1f1f1fu, kSpareBits = 0xe0e0e0e0u, kScoreMask = 0x00ffffffu;

G2048_DEV Board record_cells(const Board &raw)
{
    return Board{{raw.r[0], raw.r[1], raw.r[2] & kCellBits, raw.r[3] & kCellBits}};
}

// sum over the 16 cells of (e - 1) * 2^e (0 for an empty cell); cells must be masked (e <= 31)
G2048_DEV uint32_t potential(const Board &cells)
{
    uint32_t hi = 0, lo = 0; // sum e << e, sum 1 << e
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const uint32_t e = (cells.r[i] >> (8 * l)) & 0xffu;
            hi += e << (e & 31u);
            lo += 1u << (e & 31u);
        }
    }
    return hi - lo + count_empty(cells); // an empty cell contributed 0 - 1
}

// 12 spare bits of one register -> 12 contiguous bits
G2048_DEV uint32_t gather12(uint32_t r)
{
    uint32_t y = (r >> 5) & 0x07070707u;
    y = (y | (y >> 5)) & 0x003f003fu;
    return (y | (y >> 10)) & 0xfffu;
}

// 12 contiguous bits -> the spare bits of one register
G2048_DEV uint32_t scatter12(uint32_t v)
{
    uint32_t y = (v | (v << 10)) & 0x003f003fu;
    y = (y | (y << 5)) & 0x07070707u;
    return y << 5;
}

G2048_DEV uint32_t record_deficit(const Board &raw) { return gather12(raw.r[2]) | (gather12(raw.r[3]) << 12); }

G2048_DEV uint32_t record_score(const Board &raw)
{
    return (potential(record_cells(raw)) - record_deficit(raw)) & kScoreMask;
}

G2048_DEV Board make_record(const Board &cells, uint32_t score)
{
    const uint32_t d = (potential(cells) - score) & kScoreMask;
    return Board{{cells.r[0], cells.r[1], cells.r[2] | scatter12(d & 0xfffu), cells.r[3] | scatter12(d >> 12)}};
}

// d += inc (inc = 0 or 4, given as the spread value 0 / 0x80 for bit 2 of d) without leaving the
// spread layout: the cell bits between the deficit bits are filled with ones so that the carry runs
// through them, then the new cells are put back.
G2048_DEV void record_update(Board &raw, const Board &cells, uint32_t inc_spread)
{
    const uint64_t filled = (static_cast<uint64_t>(raw.r[3] | kCellBits) << 32) | (raw.r[2] | kCellBits);
    const uint64_t sum = filled + inc_spread;
    raw.r[0] = cells.r[0];
    raw.r[1] = cells.r[1];
    raw.r[2] = bfi(kSpareBits, static_cast<uint32_t>(sum), cells.r[2]);
    raw.r[3] = bfi(kSpareBits, static_cast<uint32_t>(sum >> 32), cells.r[3]);
}

// game2048_env.py:102-111 as a record: fresh board, score 0, so d = potential = 4 per spawned 4.
G2048_DEV Board fresh_record(uint32_t w1, uint32_t w2)
{
    Board bd = fresh_board(w1, w2);
    const uint32_t fours = (fresh_is_four_16(w1) ? 1u : 0u) + (fresh_is_four_15(w2) ? 1u : 0u);
    // d = 4 -> bit 2 of d = bit 7 of byte 8; d = 8 -> bit 3 of d = bit 5 of byte 9
    bd.r[2] |= fours == 1u ? 0x80u : (fours == 2u ? 0x2000u : 0u);
    return bd;
}

// The same through a 16-entry table of one-tile boards (entry p = a board whose only tile is a 2,
// exponent 1, in cell p): two table reads, shifts and ORs instead of ~40 VALU of placement logic.
// `Tables` supplies onehot_cell(p) (LDS on the device, an array in the host check).
template <class Tables>
G2048_DEV Board fresh_record_lut(uint32_t w1, uint32_t w2, const Tables &tb)
{
    const uint32_t p1 = w1 >> 28;                  // (w1 * 16) >> 32: cell of the first tile
    const uint32_t k2 = g2048_mulhi(w2, 15u);
    const uint32_t p2 = k2 + (k2 >= p1 ? 1u : 0u); // k2-th empty cell, skipping p1
    const uint32_t s1 = fresh_is_four_16(w1) ? 1u : 0u; // 1: the tile is a 4 (exponent 2 = 1 << 1)
    const uint32_t s2 = fresh_is_four_15(w2) ? 1u : 0u;
    const Board a = tb.onehot_cell(p1), b = tb.onehot_cell(p2);
    const uint32_t fours = s1 + s2;
    Board bd;
    bd.r[0] = (a.r[0] << s1) | (b.r[0] << s2);
    bd.r[1] = (a.r[1] << s1) | (b.r[1] << s2);
    bd.r[2] = (a.r[2] << s1) | (b.r[2] << s2) | ((fours & 1u) << 7) | ((fours >> 1) << 13); // d = 4 * fours
    bd.r[3] = (a.r[3] << s1) | (b.r[3] << s2);
    return bd;
}

// word j (0..3) of entry p of the one-tile table: 1 in byte p & 3 of register p >> 2
G2048_DEV uint32_t onehot_cell_word(uint32_t p, uint32_t j) { return (p >> 2) == j ? 1u << (8u * (p & 3u)) : 0u; }

// --------------------------------------------------------------------- stack() four cells at a time
// game2048_env.py:17-32: channel c of the observation = (cell == 2^c), i.e. (exponent == c).  All of one 32-bit word's
// four cells against one channel: t = cells ^ splat(c) has every byte < 0x40, so 0x80808080 - t has bit 7 set exactly
// in the bytes where t == 0 and no borrow crosses a byte.  An exponent >= 16 matches no channel (all-zero column).
G2048_DEV uint32_t eq_flags(uint32_t cells, uint32_t splat) { return (kHigh1 - (cells ^ splat)) & kHigh1; }             // 0x80 per match
G2048_DEV uint32_t eq_ones(uint32_t cells, uint32_t splat) { return ((kHigh1 - (cells ^ splat)) >> 7) & 0x01010101u; } // uint8 1 per match

// the same four cells as fp16 (two words: cells 0,1 and 2,3; 1.0 = 0x3c00) and fp32 (four words; 1.0 = 0x3f800000):
// the matching bytes become 0x3c / 0x3f, and v_perm puts each one in the top byte of its half / word
struct OneHot4F16 { uint32_t lo, hi; };
struct OneHot4F32 { uint32_t w[4]; };

G2048_DEV OneHot4F16 onehot4_f16(uint32_t cells, uint32_t splat)
{
    const uint32_t f = eq_flags(cells, splat);
    const uint32_t g = (f - (f >> 7)) & 0x3c3c3c3cu;
    return OneHot4F16{g2048_perm(g, g, 0x010c000cu), g2048_perm(g, g, 0x030c020cu)};
}

G2048_DEV OneHot4F32 onehot4_f32(uint32_t cells, uint32_t splat)
{
    const uint32_t f = eq_flags(cells, splat);            // 0x80 in the matching bytes: byte 2 of 1.0f
    const uint32_t g = (f - (f >> 7)) & 0x3f3f3f3fu;      // 0x3f there: byte 3 of 1.0f
    return OneHot4F32{{g2048_perm(g, f, 0x04000c0cu), g2048_perm(g, f, 0x05010c0cu), g2048_perm(g, f, 0x06020c0cu),
                       g2048_perm(g, f, 0x07030c0cu)}};
}

// One 16-byte CHUNK of a wavefront's observation piece.  The 64 boards of a wavefront are consecutive, so their
// observations are one contiguous piece of the output; the wave parks its 64 records (cells masked) in `recs` and
// writes the piece with 16-byte stores, chunk s * 64 + lane in store s (g2048_kernels.hip emit_onehot).  Per dtype:
//   OBS 0  u8 : a chunk = one channel (16 cells) of one board       16 chunks / board, boards 4s .. 4s+3 in store s
//   OBS 1  f16: a chunk = half a channel (8 cells = rows 2h, 2h+1)  32 chunks / board, boards 2s, 2s+1
//   OBS 2  f32: a chunk = one row of one channel (4 cells)          64 chunks / board, board s
// `board` = index (0..63) of the board the chunk belongs to.
struct alignas(16) Cells16 { uint32_t r[4]; };
struct alignas(16) Chunk16 { uint32_t w[4]; };

template <int OBS>
G2048_DEV Chunk16 onehot_chunk(const Cells16 *recs, uint32_t s, uint32_t lane, uint32_t &board)
{
    if constexpr (OBS == 0) {
        board = s * 4u + (lane >> 4);
        const uint32_t splat = (lane & 15u) * 0x01010101u;
        const Cells16 v = recs[board];
        return Chunk16{{eq_ones(v.r[0], splat), eq_ones(v.r[1], splat), eq_ones(v.r[2], splat), eq_ones(v.r[3], splat)}};
    } else if constexpr (OBS == 1) {
        board = s * 2u + (lane >> 5);
        const uint32_t splat = ((lane >> 1) & 15u) * 0x01010101u, half = lane & 1u;
        const OneHot4F16 a = onehot4_f16(recs[board].r[half * 2u], splat), b = onehot4_f16(recs[board].r[half * 2u + 1u], splat);
        return Chunk16{{a.lo, a.hi, b.lo, b.hi}};
    } else {
        board = s;
        const OneHot4F32 h = onehot4_f32(recs[board].r[lane & 3u], (lane >> 2) * 0x01010101u);
        return Chunk16{{h.w[0], h.w[1], h.w[2], h.w[3]}};
    }
}

// ---------------------------------------------------------------------- one env step on a record
struct StepOut {
    uint32_t gain;   // merge score of the move (:85); 0 when illegal
    bool legal;      // false = the reference's IllegalMove (:91)
    bool terminated; // :89 / :94
    uint32_t legal_mask; // all-ones when legal (lane-wide select mask, reused by reset_record)
    Board terminal;  // step_record only: record after move + spawn, before any auto-reset ("terminal" when terminated)
};

// play_record: game2048_env.py:76-100 on one board RECORD (no reset: rec is the terminal record when
// o.terminated).  w = Philox block of this transaction: word 0 = the step's
// spawn; the reset uses words 1,2 after a legal move and 0,1 after an illegal one (an illegal move
// consumes no randomness, :91-95).  The score never appears: a merge moves potential and score together,
// only a spawned 4 touches the deficit.
template <class Tables>
G2048_DEV StepOut play_record(Board &rec, uint32_t action, const Words &w, uint32_t max_exp, const Tables &tb)
{
    StepOut o;
    Board cells = record_cells(rec);
    o.legal = move_sel(cells, tb.move_sel(action), o.gain);        // :85 (illegal: board unchanged, gain 0)
    const uint32_t lm = lanemask(o.legal);
    o.legal_mask = lm;
    // :88 add_tile needs an empty cell; a board that changed always has one (a full board can only
    // change by merging).  After an illegal move nothing is spawned (:91-95).
    bool is2;                                                      // :168 the spawn's value
    const uint32_t n_empty = add_tile(cells, w.w[0], lm, is2);
    // :89 isend(): the board is full after the spawn exactly when it had one empty cell before it
    bool end = false;
    if (n_empty == 1u)                                             // :270-271
        end = !has_equal_neighbours(cells);                        // :273-280
    if (max_exp != 0 && highest(cells) == max_exp)                 // :267-268
        end = true;
    o.terminated = o.legal ? end : true;                           // :89, :94
    // a spawned 4 raises the potential without scoring: deficit += 4 (bit 2 of d = bit 7 of byte 8)
    const uint32_t inc = (o.legal && !is2) ? 0x80u : 0u;
    record_update(rec, cells, inc);
    return o;
}

// The caller's `if terminated: env.reset()` (:102-111) for a lane whose episode just ended in play_record: a
// plain divergent branch at the call site -- only the lanes that reset execute it (exec-masked writes straight
// into the record, no selects), and the wavefront skips it when none does.  The kernels store the terminal
// record BEFORE calling this, so the fresh record overwrites it in place and no second copy is ever live
// (four v_mov per lane otherwise; -0.2 us per launch at 2^20 boards, profiles/r02_s_ubench_2p20.txt).
template <class Tables>
G2048_DEV void reset_record(Board &rec, const StepOut &o, const Words &w, const Tables &tb)
{
    rec = fresh_record_lut(bfi(o.legal_mask, w.w[1], w.w[0]), bfi(o.legal_mask, w.w[2], w.w[1]), tb); // :104-109
}

// play_record + reset_record in one call, keeping the terminal record in o.terminal (host mirror, tools).
template <class Tables>
G2048_DEV StepOut step_record(Board &rec, uint32_t action, const Words &w, uint32_t max_exp, bool auto_reset,
                              const Tables &tb)
{
    StepOut o = play_record(rec, action, w, max_exp, tb);
    o.terminal = rec;
    if (o.terminated && auto_reset)
        reset_record(rec, o, w, tb);
    return o;
}

// ------------------------------------------------------- one step of the greedy n-tuple player on a record
// g2048_ntuple_play (include/g2048.h): the action of ntuple_root on the record's cells, then exactly the
// step g2048_step makes of that action -- the Philox block (t, board) of the spawn stream, board = board_offset + i, and
// play_record.  No arithmetic of its own.  w comes back for the caller's reset_record, which needs the same block.
template <uint32_t T, class Shape, class Tables>
G2048_DEV StepOut ntuple_play_step(Board &rec, uint64_t t, uint32_t board, uint32_t seed_lo, uint32_t seed_hi, const Shape &sh,
                                   uint32_t F, const int32_t *weights, uint32_t max_exp, const Tables &tb, Words &w)
{
    w = philox4x32_10(static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), board, 0u, seed_lo, seed_hi);
    const uint32_t action = ntuple_root<T>(record_cells(rec), sh, F, weights, tb).action;
    return play_record(rec, action, w, max_exp, tb);
}

// ------------------------------------------------------- tile-downgrading: a board of very large tiles, translated
// g2048_downgrade_plain / _boards / g2048_ntuple_play_downgraded (include/g2048.h; after Guei, Chen & Wu
// 2022 -- the choice of k and the guard below are this project's own).  In exponents e_c = byte & 0x1f of cell c, so the rule
// reads an engine record as well as a plain board and the score bits of a record never reach the result:
//   P = the exponents e >= 1 on the board, D = those held by two or more cells, m = max P (empty board: identity, k = 0)
//   m < min_exp: identity, k = 0
//   k = the LARGEST c with floor_exp <= c < m, c not in P and (c - 1) not in D; none: identity, k = 0
//   out_c = e_c - 1 where e_c > k, else e_c
// k is the "missing tile".  The guard on c - 1 keeps the translated board honest one move ahead: two tiles 2^(k-1) could merge
// into a real 2^k, which would sit beside the halved 2^(k+1) and look mergeable with it (deeper collisions of this kind are
// accepted).  The map is strictly increasing on the tiles of one board, so a move is legal on the translated board exactly
// where it is legal on the board, and slides and merges the same cells; only the gains of halved tiles differ.  One
// application.  Integers only, no table: P and D from 16 byte extracts, the subtraction SWAR on the four rows -- after masking
// to 5 bits, ((row + (31 - k) * 0x01010101) >> 5) & 0x01010101 is 1 exactly where e > k, and no carry crosses a byte
// (31 + 27 < 256: k >= kDowngradeMinFloor).
constexpr uint32_t kDowngradeMinFloor = 4u;  // = G2048_DOWNGRADE_MIN_FLOOR: the spawn tiles and their first merge stay below k
constexpr uint32_t kDowngradeSkipped = 0xffu; // = G2048_DOWNGRADE_SKIPPED

struct DowngradeRule {
    uint32_t min_exp;   // 1..31
    uint32_t floor_exp; // kDowngradeMinFloor..31
};

struct Downgraded {
    Board cells; // plain exponents: every byte below 32
    uint32_t k;  // the missing tile's exponent; 0: the board came through unchanged
};

G2048_DEV Downgraded downgrade_cells(const Board &raw, const DowngradeRule &rule)
{
    Downgraded out;
    uint32_t present = 0, twice = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        out.cells.r[i] = raw.r[i] & kCellBits;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const uint32_t bit = 1u << ((out.cells.r[i] >> (8 * l)) & 0x1fu);
            twice |= present & bit;
            present |= bit;
        }
    }
    present &= ~1u; // (empty cells are no tile)
    twice &= ~1u;
    const uint32_t m = 31u - g2048_clz(present | 1u); // 0 on the empty board: no candidate below it
    uint32_t cand = ~present & ~(twice << 1) & ((1u << m) - 1u) & ~((1u << rule.floor_exp) - 1u);
    cand = m < rule.min_exp ? 0u : cand;
    out.k = cand != 0u ? 31u - g2048_clz(cand) : 0u;
    const uint32_t add = (31u - out.k) * 0x01010101u, ones = out.k != 0u ? 0x01010101u : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        out.cells.r[i] -= ((out.cells.r[i] + add) >> 5) & ones;
    return out;
}

// One move of g2048_ntuple_play_downgraded on a record: ntuple_play_step with the action of ntuple_root on the TRANSLATED cells
// of the record (a staged network so takes the stage of the translated board); the record itself is stepped as before, so the
// gain, the spawn and the end of the episode are the real game's.
template <uint32_t T, class Shape, class Tables>
G2048_DEV StepOut ntuple_play_downgraded_step(Board &rec, uint64_t t, uint32_t board, uint32_t seed_lo, uint32_t seed_hi, const Shape &sh,
                                              uint32_t F, const int32_t *weights, uint32_t max_exp, const DowngradeRule &rule,
                                              const Tables &tb, Words &w)
{
    w = philox4x32_10(static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), board, 0u, seed_lo, seed_hi);
    const uint32_t action = ntuple_root<T>(downgrade_cells(rec, rule).cells, sh, F, weights, tb).action;
    return play_record(rec, action, w, max_exp, tb);
}

// ------------------------------------------------------- one fused TD step of the greedy n-tuple player on a record
// g2048_ntuple_td_step (include/g2048.h): the front half of every n-tuple learner on one record --
// ntuple_root, the step g2048_step makes of its action (the Philox block (t, board), play_record), the auto-reset, and
// ntuple_root again on the record as it then stands (the fresh board after a reset) -- with no arithmetic of its own but the
// delta, which is ntuple_trace_delta's.  ended(o, rec) is called once, behind play_record and before the reset overwrites the
// terminal record, whether the episode ended or not: the device's is wave-wide (record_episode_ends), the host's a plain copy.
//
// ntuple_root_kept is ntuple_root for a caller that uses the chosen afterstate, its value or `best`: the same keys and so the
// same choice, with what belongs to the best direction so far kept by a select per direction.  ntuple_root looks them up in
// m[action] and q[action] afterwards, and an array indexed by a run-time action lives in scratch memory on the device (176
// bytes per lane and 18 KiB of promoted LDS in the first build of ntuple_td_step_kernel); its callers so far use only
// `action`, where that look-up is dead code.  q[] is not filled in.
struct NtupleKept {
    uint32_t action;
    int64_t best;        // q[action]; 0 when no move is legal
    Board after;         // the afterstate of `action`; the board itself when no move is legal
    int64_t after_value; // V(after); 0 when no move is legal
};

template <uint32_t T, class Shape, class Tables>
G2048_DEV NtupleKept ntuple_root_kept(const Board &cells, const Shape &sh, uint32_t F, const int32_t *weights, const Tables &tb)
{
    NtupleKept r;
    r.best = 0;
    r.after = cells;
    r.after_value = 0;
    uint64_t best = 0;
#pragma nounroll // (one direction's body, four times: unrolled, the kernel holds 161 instead of 93 VGPRs at T = 4 and four times the code)
    for (uint32_t d = 0; d < 4u; ++d) {
        const NtupleMove m = ntuple_move<T>(cells, d, sh, F, weights, tb);
        const uint64_t key = ntuple_key(m.q, m.legal, d);
        if (m.legal && key > best) { // (a legal key is above every illegal one; two keys never tie: 3 - d is in them)
            r.best = m.q;
            r.after = m.after;
            r.after_value = m.v;
        }
        best = key > best ? key : best;
    }
    r.action = root_key_action(best);
    return r;
}

struct NtupleTdOut {
    uint32_t action;     // the first root's: the move played
    Board after;         // ... its afterstate, plain cells
    int64_t after_value; // ... and V of it
    int64_t best_next;   // `best` of the board after the step, not masked
    int64_t delta;       // (terminated ? 0 : best_next) - after_value
    StepOut step;
};

template <uint32_t T, class Shape, class Tables, class Ended>
G2048_DEV NtupleTdOut ntuple_td_step(Board &rec, uint64_t t, uint32_t board, uint32_t seed_lo, uint32_t seed_hi, const Shape &sh,
                                     uint32_t F, const int32_t *weights, uint32_t max_exp, const Tables &tb, Ended &&ended)
{
    NtupleTdOut out;
    {
        const NtupleKept r0 = ntuple_root_kept<T>(record_cells(rec), sh, F, weights, tb);
        out.action = r0.action;
        out.after = r0.after;
        out.after_value = r0.after_value;
    }
    const Words w = philox4x32_10(static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), board, 0u, seed_lo, seed_hi);
    out.step = play_record(rec, out.action, w, max_exp, tb);
    ended(out.step, rec);
    if (out.step.terminated)
        reset_record(rec, out.step, w, tb);
    out.best_next = ntuple_root_kept<T>(record_cells(rec), sh, F, weights, tb).best;
    out.delta = ntuple_trace_delta(out.best_next, out.after_value, out.step.terminated);
    return out;
}

// ------------------------------------------------------- the n-tuple move log and its backward error
// g2048_ntuple_play_log and g2048_ntuple_log_delta (include/g2048.h).  A log of depth M holds M + 1 slots
// of n entries, slot-major: the afterstate played, (its merge gain) << F, and a flag byte.  Slot m = 1..M of a play_log call
// is what the m-th round of g2048_ntuple_evaluate -> g2048_step wrote; slot 0 is slot M of the call before.
constexpr uint32_t kNtupleLogMaxDepth = 1024u;
constexpr uint32_t kNtupleLogValid = 1u, kNtupleLogEnded = 2u; // = G2048_NTUPLE_LOG_VALID, G2048_NTUPLE_LOG_ENDED

struct NtupleLogEntry {
    Board after;   // E.after: the afterstate of the move played; the board itself when no move is legal
    int64_t gain;  // E.best - E.after_value = (merge gain) << F; 0 when no move is legal
    uint32_t flag; // 0 when the board had no legal move, else kNtupleLogValid | (terminated ? kNtupleLogEnded : 0)
};

// One move of g2048_ntuple_play_log on a record: ntuple_play_step with ntuple_root_kept in place of ntuple_root -- the same
// keys, so the same action and the same step -- and the entry the move leaves in the log.  A root with a legal move plays a
// legal one, so `!legal` of the step is "the board had no legal move".  w comes back for the caller's reset_record.
template <uint32_t T, class Shape, class Tables>
G2048_DEV StepOut ntuple_play_log_step(Board &rec, uint64_t t, uint32_t board, uint32_t seed_lo, uint32_t seed_hi, const Shape &sh,
                                       uint32_t F, const int32_t *weights, uint32_t max_exp, const Tables &tb, Words &w, NtupleLogEntry &e)
{
    w = philox4x32_10(static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), board, 0u, seed_lo, seed_hi);
    uint32_t action;
    {
        const NtupleKept r = ntuple_root_kept<T>(record_cells(rec), sh, F, weights, tb);
        action = r.action;
        e.after = r.after;
        e.gain = static_cast<int64_t>(static_cast<uint64_t>(r.best) - static_cast<uint64_t>(r.after_value));
    }
    const StepOut o = play_record(rec, action, w, max_exp, tb);
    e.flag = o.legal ? (kNtupleLogValid | (o.terminated ? kNtupleLogEnded : 0u)) : 0u;
    return o;
}

// The backward error of slot m from the flag bytes f = flag[m], f1 = flag[m + 1] (any byte: only bits 0 and 1 are read):
//   !(f & VALID) -> 0;  f & ENDED -> 0 - V(after[m]);  !(f1 & VALID) -> 0;  else gain[m + 1] + V(after[m + 1]) - V(after[m])
// ntuple_log_reads_self: V(after[m]) is read; ntuple_log_reads_next: gain[m + 1] and V(after[m + 1]) are.  int64, wraps.
G2048_DEV bool ntuple_log_reads_self(uint32_t f, uint32_t f1)
{
    return (f & kNtupleLogValid) != 0u && ((f & kNtupleLogEnded) != 0u || (f1 & kNtupleLogValid) != 0u);
}
G2048_DEV bool ntuple_log_reads_next(uint32_t f, uint32_t f1)
{
    return (f & kNtupleLogValid) != 0u && (f & kNtupleLogEnded) == 0u && (f1 & kNtupleLogValid) != 0u;
}
// v0 = V(after[m]) where ntuple_log_reads_self, gain1 and v1 = gain[m + 1] and V(after[m + 1]) where ntuple_log_reads_next;
// what is not read is not looked at
G2048_DEV int64_t ntuple_log_delta(uint32_t f, uint32_t f1, int64_t gain1, int64_t v1, int64_t v0)
{
    if (!ntuple_log_reads_self(f, f1))
        return 0;
    const uint64_t target = ntuple_log_reads_next(f, f1) ? static_cast<uint64_t>(gain1) + static_cast<uint64_t>(v1) : 0ull;
    return static_cast<int64_t>(target - static_cast<uint64_t>(v0));
}

// ------------------------------------------------------------------- midpoint restart
// A board whose episode has just ended goes back to the middle of the run that ended, so that late-game positions are met
// more often (g2048_restart_step, include/g2048.h; the restart of Matsuzaki 2017, with snapshots every
// s = 2^k positions in place of whole recorded games).  Any network, no stage, no pool, no batch-wide rank: everything is a
// function of the one board's own history, so the bits are those of any launch geometry and of any sharding.  Integers only.
//   snap      [C][n] engine records, slot-major: slot j of board i = the record at position (j + 1) * s of the current lineage
//   pos       p: non-terminating steps since the lineage's empty board;  start  S: where the current run began (0: a fresh game)
//   restarts  restarts made so far in the lineage
// One operation, restart_board, after a step with auto-reset on:
//   terminated == 0:  pos == 2^32 - 1 -> nothing.  Else p = pos + 1; pos = p; if p & (s - 1) == 0 and 1 <= q = p >> k <= C:
//                     snap[q - 1][i] = record
//   terminated != 0 (the record is already the fresh auto-reset board):
//                     L = pos, R = L - S, m = S + (R >> 1), q = min(m >> k, C), S' = q << k
//                     if R >= min_span, restarts < max_restarts, q >= 1 and S' > S:
//                         record = snap[q - 1][i]; start = pos = S'; restarts += 1
//                     else the fresh board stays and start = pos = restarts = 0
// S' > S and S' <= m <= L: slot q - 1 was written by the current run; the slots at or below S belong to the shared prefix.  No
// slot is read that this lineage did not write, and no lane touches another board's state.
constexpr uint32_t kRestartMaxStrideLog2 = 16, kRestartMaxCapacity = 4096; // = G2048_RESTART_MAX_STRIDE_LOG2, _MAX_CAPACITY
constexpr uint32_t kRestartMinSpan = 2, kRestartMaxSpan = 0x80000000u;     // min_span in 2..2^31

struct RestartRule {
    uint32_t stride_log2, capacity, min_span, max_restarts; // k, C, min_span, max_restarts
};
// g2048_restart, checked by the caller: the rule and the state of n boards
struct Restart {
    RestartRule rule;
    uint4 *snap;                    // [C][n] records
    uint32_t *pos, *start, *restarts; // [n] each
};
// pos, start and restarts of one board, in registers
struct RestartBoard {
    uint32_t pos, start, restarts;
};

// one 16-byte record of a slot: one global_store_dwordx4 per lane, contiguous over the wave
#if defined(G2048_HOST_CHECK)
G2048_DEV void restart_store(uint4 *slot, uint32_t i, const Board &b) { __builtin_memcpy(slot + i, b.r, 16); }
#else
G2048_DEV void restart_store(uint4 *slot, uint32_t i, const Board &b) { slot[i] = make_uint4(b.r[0], b.r[1], b.r[2], b.r[3]); }
#endif

// Where restart_board finds the live record of its board: in the registers of a kernel that plays on (RestartRecordHeld), or in
// memory, read and written only where the rule asks for it (RestartRecordStored)
struct RestartRecordHeld {
    Board &rec;
    G2048_MEMBER Board get() const { return rec; }
    G2048_MEMBER void set(const Board &b) const { rec = b; }
};
struct RestartRecordStored {
    uint4 *records;
    uint32_t i;
    G2048_MEMBER Board get() const { return load_board(records, i); }
    G2048_MEMBER void set(const Board &b) const { restart_store(records, i, b); }
};

// The restart step of board i of n (the rule above).  When terminated == false only b.pos is read and written.
template <class Record>
G2048_HOST_DEV void restart_board(const Record &record, bool terminated, const RestartRule &r, uint4 *snap, uint32_t n, uint32_t i,
                                  RestartBoard &b)
{
    const uint32_t k = r.stride_log2;
    if (!terminated) {
        if (b.pos == 0xffffffffu)
            return;
        const uint32_t p = b.pos + 1u, q = p >> k;
        b.pos = p;
        if ((p & ((1u << k) - 1u)) == 0u && q >= 1u && q <= r.capacity)
            restart_store(snap + static_cast<uint64_t>(q - 1u) * n, i, record.get());
        return;
    }
    const uint32_t S = b.start, R = b.pos - S, m = S + (R >> 1);
    const uint32_t q = (m >> k) < r.capacity ? (m >> k) : r.capacity;
    const uint32_t S1 = q << k; // q <= 4096, k <= 16: below 2^29
    if (R >= r.min_span && b.restarts < r.max_restarts && q >= 1u && S1 > S) {
        record.set(load_board(snap + static_cast<uint64_t>(q - 1u) * n, i));
        b.start = b.pos = S1;
        b.restarts += 1u;
    } else {
        b.start = b.pos = b.restarts = 0u;
    }
}

// ------------------------------------------------------------------------------ one env step
struct StepResult {
    float reward;
    bool terminated;
    bool illegal;
    Board terminal;         // board the episode ended on (valid when terminated)
    int32_t terminal_score; // its final merge score
};

// Word `s` (0..3) of a Philox block without a runtime-indexed array.
G2048_DEV uint32_t select_word(const Words &w, uint32_t s)
{
    return s == 0u ? w.w[0] : (s == 1u ? w.w[1] : (s == 2u ? w.w[2] : w.w[3]));
}

// game2048_env.py:76-100 on one board, followed -- when auto_reset -- by the caller's
// `if terminated: env.reset()` (game2048_env.py:102-111).  w = Philox block of this transaction:
// word 0 = the step's spawn; the reset uses words 1,2 after a legal move and 0,1 after an illegal
// one (an illegal move consumes no randomness, game2048_env.py:91-95).
G2048_DEV StepResult step_env(Board &bd, int32_t &score, uint32_t action, const Words &w, float illegal_reward,
                              uint32_t max_exp, bool auto_reset)
{
    StepResult r;
    uint32_t gain;
    const bool legal = move(bd, action, gain);            // :85 (an illegal move leaves bd unchanged
                                                          //      and merges nothing: gain == 0)
    // :88 add_tile needs an empty cell; a board that changed always has one (a full board can only
    // change by merging).  After an illegal move nothing is spawned (:91-95).
    const uint32_t n_empty = add_tile(bd, w.w[0], lanemask(legal));
    // :89 isend(): the board is full after the spawn exactly when it had one empty cell before it
    bool end = false;
    if (n_empty == 1u)                                    // :270-271
        end = !has_equal_neighbours(bd);                  // :273-280
    if (max_exp != 0 && highest(bd) == max_exp)           // :267-268
        end = true;
    r.illegal = !legal;                                   // :91-95
    r.terminated = legal ? end : true;
    r.reward = legal ? (float)gain : illegal_reward;      // :90 / :95
    score += (int32_t)gain;                               // :86
    r.terminal = bd;
    r.terminal_score = score;
    const bool do_reset = r.terminated && auto_reset;
    if (g2048_any(do_reset)) {                            // wave-uniform: skipped when nobody finished
        const uint32_t lm = lanemask(legal), rm = lanemask(do_reset);
        const Board fb = fresh_board(bfi(lm, w.w[1], w.w[0]), bfi(lm, w.w[2], w.w[1])); // :104,:108-109
        bd.r[0] = bfi(rm, fb.r[0], bd.r[0]);
        bd.r[1] = bfi(rm, fb.r[1], bd.r[1]);
        bd.r[2] = bfi(rm, fb.r[2], bd.r[2]);
        bd.r[3] = bfi(rm, fb.r[3], bd.r[3]);
        score &= (int32_t)~rm;                            // :105
    }
    return r;
}

} // namespace g2048
