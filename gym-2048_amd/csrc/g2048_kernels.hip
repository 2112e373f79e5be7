// g2048_kernels.hip -- gfx950 (MI355X / CDNA4) kernels of the batched 2048 environment.
//
// Mapping: ONE BOARD PER LANE.  A wavefront owns 64 consecutive boards = 1 KiB of board records, read
// and written with one global_load/store_dwordx4 per lane (fully coalesced, 16 B/lane).  The whole
// step -- slide/merge sweep, score, spawn, done detection -- runs out of VGPRs with byte-parallel
// integer ops (g2048_device.h); there is no per-board RNG state: the spawn randomness of
// (transaction t, board b) is one Philox4x32-10 block.
//
// HBM bytes per env-step of step_kernel (the roofline figure in DESIGN.md):
//   algorithmic 38 B = board in 16 + action 1 + board out 16 + reward 4 + terminated 1
// and that is also all a step moves for a board whose episode goes on: the episodic score travels
// inside the 16-byte record (g2048_device.h "board RECORD").  A board whose episode ENDS additionally
// writes its terminal record to last_record (sparse 16-byte store; the episode's return is computed
// from it when somebody asks) unless the engine was told not to keep them (g2048_set_last_records: 0.85 us
// of a 10.2 us launch at 2^20 boards, tools/ubench/r4_probe.hip), and every wavefront adds its counts and the
// merge scores of its 64 moves to its 32-byte slot (12 bytes stored per launch).
#include "g2048_kernels.h"

#include "g2048_device.h"
#include "g2048_pcg64.h"

#include <atomic>
#include <type_traits>


namespace g2048 {

constexpr int kBlock = 256;

// Streaming accesses of the step kernels carry the non-temporal hint (nt=1): every byte is touched
// exactly once per launch, so it should not displace anything in L2 / Infinity Cache.  Measured on
// MI355X (tools/ubench/step_variants.hip, v14): 2^24 boards 181 -> 128 us per launch, 2^20 boards
// 10.9 -> 10.5 us.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ Board load_board_nt(const uint4 *boards, uint32_t i)
{
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(boards) + i);
    return Board{{v.x, v.y, v.z, v.w}};
}

__device__ __forceinline__ void store_board_nt(uint4 *boards, uint32_t i, const Board &b)
{
    const u32x4 v = {b.r[0], b.r[1], b.r[2], b.r[3]};
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(boards) + i);
}

// one 16-byte piece of an observation: written once and read by somebody else's kernel, so a streaming (nt) store
__device__ __forceinline__ void store_chunk_nt(uint4 *out, uint64_t g, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const u32x4 v = {a, b, c, d};
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(out) + g);
}

__device__ __forceinline__ void store_board(uint4 *boards, uint32_t i, const Board &b)
{
    boards[i] = make_uint4(b.r[0], b.r[1], b.r[2], b.r[3]);
}

// Per-WAVEFRONT lookup tables in LDS (512 B): the per-action selector rows of move_sel and the 16
// one-tile boards of fresh_record_lut (g2048_device.h).  Each wavefront stages its own copy -- every lane
// fetches ONE 8-byte piece of the 512-byte image below (global load, L2-resident) and writes it to LDS at
// byte offset threadIdx.x * 8 -- and only reads what it wrote itself, so no workgroup barrier is involved.
struct WaveTables {
    uint32_t move[32]; // 4 actions x 8 words (6 used)
    uint32_t cell[64]; // 16 cells x 4 words: entry p = the board whose only tile is a 2 (exponent 1) in cell p
    uint32_t pad[32];  // 64 lanes x 8 bytes
};

// word j of entry p of the one-tile table (= onehot_cell_word(p, j) of g2048_device.h, as a constant expression)
#define G2048_CELL_ENTRY(p) ((p) / 4 == 0 ? 1u << (8 * ((p) % 4)) : 0u), ((p) / 4 == 1 ? 1u << (8 * ((p) % 4)) : 0u), \
                            ((p) / 4 == 2 ? 1u << (8 * ((p) % 4)) : 0u), ((p) / 4 == 3 ? 1u << (8 * ((p) % 4)) : 0u)
__device__ const uint32_t kWaveTablesImage[128] __attribute__((aligned(16))) = {
    G2048_MOVE_LUT_WORDS,
    G2048_CELL_ENTRY(0), G2048_CELL_ENTRY(1), G2048_CELL_ENTRY(2), G2048_CELL_ENTRY(3),
    G2048_CELL_ENTRY(4), G2048_CELL_ENTRY(5), G2048_CELL_ENTRY(6), G2048_CELL_ENTRY(7),
    G2048_CELL_ENTRY(8), G2048_CELL_ENTRY(9), G2048_CELL_ENTRY(10), G2048_CELL_ENTRY(11),
    G2048_CELL_ENTRY(12), G2048_CELL_ENTRY(13), G2048_CELL_ENTRY(14), G2048_CELL_ENTRY(15),
    /* pad[32] = 0 */
};
#undef G2048_CELL_ENTRY

// `x`, but not before `dep` has been computed (pins the s_waitcnt of a load below independent work).
__device__ __forceinline__ uint2 use_after(uint2 x, uint32_t dep)
{
    unsigned long long both = (static_cast<unsigned long long>(x.y) << 32) | x.x; // ONE 64-bit operand: the pair stays a pair
    asm volatile("" : "+v"(both) : "v"(dep));
    return make_uint2(static_cast<uint32_t>(both), static_cast<uint32_t>(both >> 32));
}

struct LdsTables {
    const WaveTables *t;
    __device__ __forceinline__ MoveSel move_sel(uint32_t action) const
    {
        const uint4 a = *reinterpret_cast<const uint4 *>(t->move + action * 8u);
        const uint2 b = *reinterpret_cast<const uint2 *>(t->move + action * 8u + 4u);
        return MoveSel{a.x, a.y, a.z, a.w, b.x, b.y};
    }
    __device__ __forceinline__ Board onehot_cell(uint32_t p) const
    {
        const uint4 v = *reinterpret_cast<const uint4 *>(t->cell + p * 4u);
        return Board{{v.x, v.y, v.z, v.w}};
    }
};

// Two halves so that the global load is issued early and waited for late (after the Philox block).
__device__ __forceinline__ uint2 load_tables_piece()
{
    return reinterpret_cast<const uint2 *>(kWaveTablesImage)[threadIdx.x & 63u];
}

__device__ __forceinline__ LdsTables stage_tables(WaveTables *all, uint2 piece)
{
    // wave w's copy starts at w * 512 bytes and lane l writes bytes [8l, 8l + 8): together threadIdx.x * 8
    reinterpret_cast<uint2 *>(all)[threadIdx.x] = piece;
    // same-wave LDS writes are visible to the wave's later reads in program order; the fence only
    // keeps the compiler from moving those reads up
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return LdsTables{all + (threadIdx.x >> 6)};
}

// One lane of a one-board-per-lane launch.  Lanes past the end stay active (whole wavefronts for the ballots and the
// DPP sums): they recompute board n - 1 and write nothing.
// FULL: the batch is a whole number of blocks, no lane is past the end -- `valid` is a compile-time true.
struct Lane { uint32_t i_raw, i; bool valid; }; // blockIdx.x * BLOCK + threadIdx.x; the board worked on; i_raw < n
template <uint32_t BLOCK, bool FULL> __device__ __forceinline__ Lane lane_of(uint32_t n)
{
    const uint32_t i_raw = blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = FULL || i_raw < n;
    return Lane{i_raw, valid ? i_raw : n - 1u, valid};
}

// ---- actions.  ACT: 0 = the synthetic policy (no buffer: the top two bits of the step's Philox word 3), 1 / 2 / 3 = a
// buffer of uint8 / int32 / int64.  A loaded action keeps its memory type until it is consumed: the fused rollout holds
// its actions in flight for kPrefetch steps, and a conversion next to the load would be a use of its result (the wait
// would land there instead of kPrefetch steps later).
template <int ACT> struct RawAction { typedef uint32_t type; };
template <> struct RawAction<1> { typedef uint8_t type; };
template <> struct RawAction<2> { typedef int32_t type; };
template <> struct RawAction<3> { typedef long long type; };
template <int ACT>
__device__ __forceinline__ typename RawAction<ACT>::type load_action_at(const void *__restrict__ actions, size_t idx)
{
    if constexpr (ACT == 0)
        return 0u;
    else
        return __builtin_nontemporal_load(static_cast<const typename RawAction<ACT>::type *>(actions) + idx);
}

// the move always uses the low two bits
template <class Raw> __device__ __forceinline__ uint32_t action_bits(Raw raw) { return static_cast<uint32_t>(raw) & 3u; }

// One lane of the wavefront (the first offender) publishes {bit 63, low byte of the action, global board index} to the
// engine's pinned error word; the host finds it at the entry of its next call on the engine.  Whole wavefronts call this.
__device__ __forceinline__ void report_bad_action(unsigned long long *action_err, bool bad, uint32_t raw_low, uint32_t global_index)
{
    const unsigned long long offenders = __builtin_amdgcn_ballot_w64(bad);
    if (offenders == 0ull)
        return;
    if ((threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(offenders)))
        __hip_atomic_store(action_err, (1ull << 63) | (static_cast<unsigned long long>(raw_low & 0xffu) << 32) | global_index,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Strict actions (g2048_set_strict_actions; game2048_env.py:49 declares Discrete(4), :210-212 happens to play 4 as "down" and
// -1 as "right"): whether an action lay outside 0..3 as the RAW value of its type, and its low bits for the report.
struct BadAction {
    bool bad = false; uint32_t raw = 0;
    template <class Raw> __device__ __forceinline__ static bool outside(Raw v) // THE definition (one inline copy: rollout_fused_numpy_kernel)
    {
        typedef typename std::make_unsigned<Raw>::type U;
        return static_cast<U>(v) > static_cast<U>(3);
    }
    // ONE-SHOT, the lane's only action of a per-step launch: OVERWRITES an earlier finding (a loop over k actions needs a
    // select per action: rollout_fused_kernel).  Returns the move.  Widened first: the value is consumed at once.
    template <class Raw> __device__ __forceinline__ uint32_t note_only(Raw v)
    {
        const auto w = static_cast<typename std::conditional<(sizeof(Raw) > 4), unsigned long long, uint32_t>::type>(v);
        bad = outside(w);
        raw = static_cast<uint32_t>(w);
        return action_bits(w);
    }
};

// Episode bookkeeping, shared by every step kernel.  A lane whose episode ended stores the record it
// ended on (sparse 16-byte store; plain, not nt: L2 merges these into lines) and, if asked, the plain
// terminal board; the wave's two counts go to its slot (flush_episode_counts).  Skipped
// entirely by a wave-uniform branch when no lane terminated.
// Returns the lane mask of the boards whose episode ended in this step.
__device__ __forceinline__ unsigned long long record_episode_ends(const StepArgs &p, uint32_t i, bool fin, bool illegal,
                                                                  const Board &terminal, uint32_t &episodes, uint32_t &illegal_ends)
{
    const unsigned long long done = __builtin_amdgcn_ballot_w64(fin);
    if (done == 0ull)
        return 0ull;
    if (fin) {
        if (p.st.last_record) // (wave-uniform; NULL = the engine does not keep terminal records, g2048_set_last_records)
            store_board(p.st.last_record, i, terminal);
        if (p.terminal_boards)
            store_board(p.terminal_boards, i, record_cells(terminal));
    }
    episodes += static_cast<uint32_t>(__popcll(done));
    illegal_ends += static_cast<uint32_t>(__popcll(__builtin_amdgcn_ballot_w64(fin && illegal)));
    return done;
}

// ---- wave-wide sums.  gfx9 DPP: an inclusive scan inside each row of 16 lanes (row_shr 1, 2, 4, 8), then lane 15 of
// rows 0 / 2 is added to rows 1 / 3 (row_bcast:15) and lane 31 to rows 2, 3 (row_bcast:31): six v_add_u32_dpp, the
// wave's total ends up in LANE 63 (the other lanes hold partial sums).  Every lane of the wavefront must be active.
__device__ __forceinline__ uint32_t wave_sum_lane63(uint32_t v)
{
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x111, 0xf, 0xf, false)); // row_shr:1
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x112, 0xf, 0xf, false)); // row_shr:2
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x114, 0xf, 0xf, false)); // row_shr:4
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x118, 0xf, 0xf, false)); // row_shr:8
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x142, 0xa, 0xf, false)); // row_bcast:15 -> rows 1, 3
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x143, 0xc, 0xf, false)); // row_bcast:31 -> rows 2, 3
    return v;
}

// The same for 64-bit lane values (the gains a lane accumulated over a fused rollout): three 22-bit pieces, each of
// whose 64-lane sums fits 32 bits, recombined in lane 63.  Once per launch.
__device__ __forceinline__ unsigned long long wave_sum64_lane63(unsigned long long v)
{
    const uint32_t s0 = wave_sum_lane63(static_cast<uint32_t>(v) & 0x3fffffu);
    const uint32_t s1 = wave_sum_lane63(static_cast<uint32_t>(v >> 22) & 0x3fffffu);
    const uint32_t s2 = wave_sum_lane63(static_cast<uint32_t>(v >> 44));
    return static_cast<unsigned long long>(s0) + (static_cast<unsigned long long>(s1) << 22) +
           (static_cast<unsigned long long>(s2) << 44);
}

// ---- the wavefront's episode SLOT: 32 bytes per 64 boards (g2048_kernels.h kSlotWords), four 64-bit quantities
//   episodes      finished episodes
//   illegal_ends  ... of which ended on an illegal move
//   gain_sum      G: merge score of every move of these 64 boards since the statistics were cleared (+ the scores
//                 they held then, -/+ what g2048_reset / g2048_set_scores took away or put in).  Conservation:
//                 every point scored is either still on a live board or belongs to a finished episode, so
//                     sum of the final scores of ALL finished episodes  =  G - sum of the live boards' scores
//                 which the statistics kernel evaluates (g2048_stats.return_sum) -- exact, and no per-episode
//                 work in the step: the step only adds its 64 gains (six DPP adds)
//   pending       bit l: board l's episode has ended and the board has NOT been reset (auto_reset == 0): its score
//                 belongs to a finished episode although it is still in the record
// stored as EIGHT DWORDS with the four LOW halves first: {episodes.lo, illegal_ends.lo, gain_sum.lo, pending.lo,
// episodes.hi, illegal_ends.hi, gain_sum.hi, pending.hi}.  Sparse stores cost per DWORD on this chip (the 16-byte
// terminal-record store of 7 % of the lanes costs 0.57 us per launch at 2^20 boards, a 4-byte one 0.11 us,
// profiles/r02_g_ubench_2p20.txt; storing all eight dwords of the slot per launch measured +0.32 us against the two-word
// slot of round 3, tools/ubench/r4_probe.hip), so a launch stores the THREE low counter dwords with one
// global_store_dwordx3 and touches the rest only when it changes: the high halves on a carry (once in 2^32 counts), the
// pending mask when it differs from the one that came in (never with auto_reset).
// The slot is private to its wavefront (one wavefront per slot per launch, launches are stream-ordered), so it is
// updated without atomics: the old values come in through the SCALAR cache (uniform address, one s_load_dwordx8 at
// kernel entry -- no VALU, no vector-memory instruction, latency never exposed) and ONE lane -- lane 63, where the DPP
// sum of the gains lands -- stores the new ones.  Measured against 64-bit atomics: -0.5 us per launch at 2^20 boards
// (profiles/r02_g_ubench_2p20.txt).
struct EpisodeCounters {
    uint32_t *slot;
    uint32_t ep_lo, ill_lo, gain_lo, pend_lo, ep_hi, ill_hi, gain_hi, pend_hi;
};

__device__ __forceinline__ uint32_t *slot_of(unsigned long long *ep_counters, uint32_t wave_id)
{
    return reinterpret_cast<uint32_t *>(ep_counters + kSlotWords * wave_id);
}

__device__ __forceinline__ EpisodeCounters load_episode_counters(const StepArgs &p, uint32_t i_raw)
{
    uint32_t *slot = slot_of(p.st.ep_counters, __builtin_amdgcn_readfirstlane(i_raw >> 6));
    const uint4 lo = *reinterpret_cast<const uint4 *>(slot), hi = *reinterpret_cast<const uint4 *>(slot + 4);
    return EpisodeCounters{slot, lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

// 64-bit views of a slot for the kernels off the hot path
__device__ __forceinline__ unsigned long long slot_get(const uint32_t *slot, uint32_t k)
{
    return static_cast<unsigned long long>(slot[k]) | (static_cast<unsigned long long>(slot[4u + k]) << 32);
}

__device__ __forceinline__ void slot_set(uint32_t *slot, uint32_t k, unsigned long long v)
{
    slot[k] = static_cast<uint32_t>(v);
    slot[4u + k] = static_cast<uint32_t>(v >> 32);
}

enum : uint32_t { kSlotEpisodes = 0, kSlotIllegal = 1, kSlotGain = 2, kSlotPending = 3 };

// gain_lane63: the wave's summed merge score of this launch, valid in lane 63 (wave_sum_lane63 / wave_sum64_lane63);
// pending: the new pending mask (wave-uniform).
__device__ __forceinline__ void flush_episode_counts(const EpisodeCounters &c, uint32_t episodes, uint32_t illegal_ends,
                                                     unsigned long long gain_lane63, unsigned long long pending)
{
    if ((threadIdx.x & 63u) != 63u)
        return;
    const unsigned long long ep = (static_cast<unsigned long long>(c.ep_hi) << 32 | c.ep_lo) + episodes;      // scalar
    const unsigned long long ill = (static_cast<unsigned long long>(c.ill_hi) << 32 | c.ill_lo) + illegal_ends; // scalar
    const unsigned long long gain = (static_cast<unsigned long long>(c.gain_hi) << 32 | c.gain_lo) + gain_lane63;
    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
    const u32x3 lo = {static_cast<uint32_t>(ep), static_cast<uint32_t>(ill), static_cast<uint32_t>(gain)};
    *reinterpret_cast<u32x3 *>(c.slot) = lo;                                           // the common case: 12 bytes
    const uint32_t ep_hi = static_cast<uint32_t>(ep >> 32), ill_hi = static_cast<uint32_t>(ill >> 32),
                   gain_hi = static_cast<uint32_t>(gain >> 32);
    if (ep_hi != c.ep_hi || ill_hi != c.ill_hi || gain_hi != c.gain_hi) {             // a carry: once in 2^32 counts
        const u32x3 hi = {ep_hi, ill_hi, gain_hi};
        *reinterpret_cast<u32x3 *>(c.slot + 4) = hi;
    }
    const uint32_t pend_lo = static_cast<uint32_t>(pending), pend_hi = static_cast<uint32_t>(pending >> 32);
    if (pend_lo != c.pend_lo || pend_hi != c.pend_hi) {                                // only without auto_reset
        c.slot[3] = pend_lo;
        c.slot[7] = pend_hi;
    }
}

// "episode ended and not reset" mask of a step launch from the mask of the lanes whose episode ended: every board was
// stepped, so older marks are gone, and with auto_reset nothing stays pending.  Scalar arithmetic, no branch.
__device__ __forceinline__ unsigned long long pending_after_step(unsigned long long done, uint32_t auto_reset)
{
    return done & (0ull - static_cast<unsigned long long>(auto_reset == 0u ? 1u : 0u));
}

// What a reset / score import does to the slot of its wavefront (not hot; whole wavefronts must call it):
//   reset of a board whose episode is still running   -> the episode is ABANDONED: its score leaves G
//   reset of a board whose episode has ended (pending) -> the mark is cleared, its score stays in G (a finished episode)
// `delta`: signed change of the board's live score caused by this call (0 for lanes that do nothing), `clear`: the lane
// clears its pending mark.
__device__ __forceinline__ void adjust_slot(unsigned long long *ep_counters, uint32_t i_raw, int32_t delta, bool clear)
{
    const uint32_t total = wave_sum_lane63(static_cast<uint32_t>(delta)); // |sum| <= 64 * 2^24: fits int32
    const unsigned long long cleared = __builtin_amdgcn_ballot_w64(clear);
    if ((threadIdx.x & 63u) == 63u) {
        uint32_t *slot = slot_of(ep_counters, i_raw >> 6);
        slot_set(slot, kSlotGain, slot_get(slot, kSlotGain) + static_cast<unsigned long long>(static_cast<long long>(static_cast<int32_t>(total))));
        slot_set(slot, kSlotPending, slot_get(slot, kSlotPending) & ~cleared);
    }
}

__device__ __forceinline__ bool is_pending(unsigned long long *ep_counters, uint32_t i_raw)
{
    const unsigned long long pending = slot_get(slot_of(ep_counters, __builtin_amdgcn_readfirstlane(i_raw >> 6)), kSlotPending);
    return ((pending >> (threadIdx.x & 63u)) & 1ull) != 0ull;
}

// ------------------------------------------------------------ observation fused into the step
// stack() (game2048_env.py:17-32) of the record a step leaves behind -- what Game2048Env.step returns first
// (game2048_env.py:100) -- written by the step kernel itself: no second launch and no re-read of the records.
//
// The 64 boards of a wavefront are consecutive, so their observations are ONE contiguous piece of the output
// (16 / 32 / 64 KiB for u8 / f16 / f32).  The wave parks its 64 records in LDS (1 KiB) and writes that piece
// with fully coalesced 16-byte streaming stores: in store s, lane l writes chunk s * 64 + l.  Per dtype a chunk is
//   u8 : one channel (16 cells) of one board      -> needs the whole record     (ds_read_b128, 4 boards per store)
//   f16: half a channel (8 cells)                 -> two words of the record    (ds_read_b64,  2 boards per store)
//   f32: one row of one channel (4 cells)         -> one word of the record     (ds_read_b32,  1 board per store)
// The byte compares (eq_ones / onehot4_f16 / onehot4_f32) live in g2048_device.h, where the host unit test reaches them.
// Occupancy of the kernels that write observations is CAPPED at 2 workgroups (8 wavefronts) per CU by launching
// them with this much unused dynamic LDS (6 KiB static + 58 KiB = 64 KiB per workgroup of the CU's 160 KiB).  The
// kernel is bound by DRAM writes, and every resident wavefront owns its own 16-64 KiB output region: with all 32
// wave slots of a CU filled the chip writes into 8 192 regions at once (128 MiB of open write window at u8) and the
// memory system runs at 5.1 TB/s; narrowing the window to 2 048 regions brings 5.9-6.1 TB/s (u8, 2^20 and 2^22
// boards: 60.5 -> 52.6 us and 239 -> 201 us; f16 103 -> 99 us; f32 is insensitive; tools/ubench/r3_probe.hip parts B
// and C, profiles/r03_d_probe_*.txt, r03_l_probe_c_*.txt; at 2^24 boards 3-4 workgroups per CU are ~3 % better
// than 2, all of them 4-9 % better than uncapped).  The arithmetic needs a sixth of the issue slots, so nothing is
// lost on the compute side.
constexpr uint32_t kObsOccupancyPad = 58u * 1024u;

// The pad plus the kernel's static LDS (the per-wave tables and the parked records) must fit the 64 KiB a workgroup may
// own; two such workgroups then fill 128 of the CU's 160 KiB and a third does not fit.
static_assert(sizeof(WaveTables) * (kBlock / 64) + sizeof(uint4) * kBlock + kObsOccupancyPad <= 64u * 1024u,
              "static LDS + occupancy pad exceed the 64 KiB workgroup limit");

// Dynamic LDS above 48 KiB is opt-in per kernel and per device.  Returns the pad to launch with: kObsOccupancyPad where
// the device granted it, 0 where it did not (a part with less LDS, a runtime that refuses) -- the kernel is then merely
// not occupancy-capped, instead of every observation-writing launch failing.  Asked once per kernel and device.
template <auto Kernel>
static uint32_t obs_pad_for()
{
    static std::atomic<signed char> state[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
        dev = 0;
    // (launches come from several threads -- two chains, LocalShards: the per-device answer is an atomic; two threads that
    //  both find it unset both ask the runtime, which is idempotent)
    signed char known = state[dev].load(std::memory_order_acquire);
    if (known == 0) {
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   static_cast<int>(kObsOccupancyPad));
        if (err != hipSuccess)
            (void)hipGetLastError(); // not sticky: the launch below goes ahead without the pad
        known = err == hipSuccess ? 1 : -1;
        state[dev].store(known, std::memory_order_release);
    }
    return known > 0 ? kObsOccupancyPad : 0u;
}

template <int OBS, bool FULL>
__device__ __forceinline__ void emit_onehot_as(const Cells16 *recs, uint4 *out, uint32_t lane, uint32_t n_here)
{
    constexpr uint32_t kStores = 16u << OBS; // 16 / 32 / 64 KiB per wavefront
    constexpr uint32_t kUnroll = OBS == 2 ? 16u : kStores;
#pragma unroll kUnroll
    for (uint32_t s = 0; s < kStores; ++s) {
        uint32_t b;
        const Chunk16 c = onehot_chunk<OBS>(recs, s, lane, b);
        if (FULL || b < n_here)
            store_chunk_nt(out, s * 64u + lane, c.w[0], c.w[1], c.w[2], c.w[3]);
    }
}

template <bool FULL>
__device__ __forceinline__ void emit_onehot(uint4 *wave_recs, const Board &rec, void *obs, uint32_t obs_dtype,
                                            uint32_t wave_first, uint32_t n)
{
    const uint32_t lane = threadIdx.x & 63u;
    wave_recs[lane] = make_uint4(rec.r[0], rec.r[1], rec.r[2] & kCellBits, rec.r[3] & kCellBits);
    // same-wave LDS accesses execute in program order; the fences keep the compiler from reordering them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // boards of this wave that exist (ragged last block only)
    const uint32_t n_here = FULL ? 64u : (wave_first < n ? (n - wave_first < 64u ? n - wave_first : 64u) : 0u);
    const Cells16 *recs = reinterpret_cast<const Cells16 *>(wave_recs);
    // the wave's piece starts at board wave_first: 16 << dtype chunks of 16 bytes per board
    uint4 *out = static_cast<uint4 *>(obs) + (static_cast<uint64_t>(wave_first) << (4u + obs_dtype));
    if (obs_dtype == 0u)
        emit_onehot_as<0, FULL>(recs, out, lane, n_here);
    else if (obs_dtype == 1u)
        emit_onehot_as<1, FULL>(recs, out, lane, n_here);
    else
        emit_onehot_as<2, FULL>(recs, out, lane, n_here);
}

// ------------------------------------------------------------------- host-visible completion
// g2048_step_host / g2048_fetch_host: the outputs of a launch live in mapped, coherent pinned HOST memory and the host
// polls one word instead of calling into the runtime (hipStreamSynchronize costs ~5 us more per call than a poll,
// tools/ubench/host_latency.hip).  A ONE-block launch publishes the word itself: every wave makes its stores visible
// at system scope, the block meets, one lane stores the value with release semantics.  Larger launches are followed
// by signal_kernel on the same stream (the kernel boundary orders it behind the outputs).
__device__ __forceinline__ void signal_done(unsigned long long *done_seq, unsigned long long value)
{
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0 && gridDim.x == 1)
        __hip_atomic_store(done_seq, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(64) signal_kernel(unsigned long long *done_seq, unsigned long long value)
{
    if (threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(done_seq, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------- stream-to-stream ordering by flags
// The two chains of a rollout (g2048_set_chains) are ordered against the caller's stream with a pair of one-wave kernels
// instead of HIP events: flag_set_kernel publishes a ticket in device memory (agent-scope release: it runs behind the
// work it stands for, in stream order), flag_wait_kernel on the other stream spins until the ticket is there (agent-scope
// acquire) and the kernels behind it follow in stream order.  An event record + hipStreamWaitEvent pair costs this
// runtime ~15 us of latency per crossing; the flag pair a few us (tools/chain_fixed_cost.py).  The wait is BOUNDED
// (2^26 polls of ~1 us, one to two minutes -- longer than any work a caller could reasonably have queued ahead of the
// ticket): a ticket that never comes must not hang the device for good.  A wait that runs out is LOUD: it publishes the
// ticket it gave up on in `timed_out` -- a word of pinned, coherent host memory the library checks at the entry of every
// call on the engine, which then fails with G2048_ERR_HIP -- because the kernels behind it run unordered against the
// other chain from there on.
__global__ void __launch_bounds__(64) flag_set_kernel(unsigned long long *flag, unsigned long long value)
{
    if (threadIdx.x == 0)
        __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(64) flag_wait_kernel(const unsigned long long *flag, unsigned long long value,
                                                       unsigned long long *timed_out, uint32_t max_polls)
{
    if (threadIdx.x != 0)
        return;
    for (uint32_t spin = 0; spin < max_polls; ++spin) {
        if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= value)
            return;
        __builtin_amdgcn_s_sleep(16); // ~1 us between polls
    }
    if (timed_out)
        __hip_atomic_store(timed_out, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------- step
// Game2048Env.step for every board (game2048_env.py:76-100), one launch per environment step.
//
// One board per lane, one pass: load the 16-byte record + the action -> Philox block (independent of
// the loads, so it runs while they are in flight) -> play_record (move through the lane's selector row,
// spawn, done detection, deficit update, auto-reset through the one-tile table) -> store record, reward,
// terminated.  No barrier, no cross-wave traffic.
// FULL: the batch is a whole number of blocks (n % 256 == 0), no lane is past the end.
//
// Kernel arguments are FLAT and ordered by need: the library is built with -mllvm -amdgpu-kernarg-preload-count=16,
// so the command processor hands the first 14 dwords (what the loads and the Philox block need) to every
// wavefront in SGPRs -- the board load is addressed without an s_load + wait on the kernarg segment.  The rest
// (outputs, written last) comes in as one by-reference struct.  -0.25 us per launch at 2^20 boards against the
// single-struct signature (profiles/r02_v_ubench_2p20.txt).
struct StepTail {
    uint8_t *terminated;
    uint4 *last_record;
    uint8_t *illegal;
    uint8_t *highest;
    uint4 *terminal_boards;
    float illegal_reward;
    uint32_t max_exp;
    uint32_t auto_reset;
    void *obs;          // HAS_OBS kernels only
    uint32_t obs_dtype;
    uint4 *boards_out;  // !STD kernels only
    unsigned long long *done_seq;
    unsigned long long done_value;
    unsigned long long *action_err; // !STD kernels only: strict actions (NULL = not checked)
};

// StepArgs -> StepTail (launchers) and back (step_body; obs, boards_out, done_* and action_err are read from the tail
// itself): a field added to one direction belongs in the other.
static StepTail step_tail(const StepArgs &a)
{
    return StepTail{a.terminated, a.st.last_record, a.illegal, a.highest, a.terminal_boards, a.illegal_reward, a.max_exp,
                    a.auto_reset, a.obs, a.obs_dtype, a.boards_out, a.done_seq, a.done_value, a.action_err};
}

// STD: the optional outputs are compile-time NULL and max_exp a compile-time 0 (no max tile), so none of their "is this
// wanted" branches exists
template <bool STD> __device__ __forceinline__ StepArgs
step_args(uint4 *boards, const void *actions, unsigned long long *ep_counters, uint32_t board_offset, uint32_t seed_lo, uint32_t seed_hi,
          uint32_t t_lo, uint32_t t_hi, uint32_t n, float *reward, const StepTail &tail)
{
    StepArgs p{};
    p.st.boards = boards;
    p.st.last_record = tail.last_record;
    p.st.ep_counters = ep_counters;
    p.actions = actions;
    p.reward = reward;
    p.terminated = tail.terminated;
    p.illegal = STD ? nullptr : tail.illegal;
    p.highest = STD ? nullptr : tail.highest;
    p.terminal_boards = STD ? nullptr : tail.terminal_boards;
    p.n = n;
    p.board_offset = board_offset;
    p.seed_lo = seed_lo;
    p.seed_hi = seed_hi;
    p.t_lo = t_lo;
    p.t_hi = t_hi;
    p.illegal_reward = tail.illegal_reward;
    p.max_exp = STD ? 0u : tail.max_exp;
    p.auto_reset = tail.auto_reset;
    return p;
}

// STD: the standard configuration -- reward and terminated present, no illegal / highest / terminal_boards, no
// max_tile -- so none of the "is this wanted" branches exists (a taken scalar branch costs a wavefront ~20 cycles).
// HAS_OBS: the step also returns its observation (game2048_env.py:100 `return stack(self.Matrix), ...`): the
// one-hot of the record it leaves behind is written by emit_onehot (+256 / 512 / 1 024 B per board; the dtype is a
// wave-uniform switch, one taken branch against hundreds of store-bound instructions).
template <int ACT, bool FULL, bool STD, bool HAS_OBS>
__device__ __forceinline__ void step_body(WaveTables *s_tables, uint4 *s_recs, uint4 *boards, const void *actions,
                                          unsigned long long *ep_counters, uint32_t board_offset, uint32_t seed_lo, uint32_t seed_hi,
                                          uint32_t t_lo, uint32_t t_hi, uint32_t n, float *reward, const StepTail &tail)
{
    const StepArgs p = step_args<STD>(boards, actions, ep_counters, board_offset, seed_lo, seed_hi, t_lo, t_hi, n, reward, tail);
    const Lane ln = lane_of<kBlock, FULL>(p.n);
    Board rec = load_board_nt(p.st.boards, ln.i);
    const uint2 tables_piece = load_tables_piece();
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);

    const Words w = philox4x32_10(p.t_lo, p.t_hi, p.board_offset + ln.i, 0u, p.seed_lo, p.seed_hi);
    BadAction bad; // (reported by the !STD kernels only)
    const uint32_t action = ACT == 0 ? w.w[3] >> 30 : bad.note_only(load_action_at<ACT>(p.actions, ln.i));
    const LdsTables tb = stage_tables(s_tables, use_after(tables_piece, w.w[0]));

    const StepOut o = play_record(rec, action, w, p.max_exp, tb);

    // episode ends first: the terminal record goes out before the reset overwrites it in place
    uint32_t episodes = 0, illegal_ends = 0;
    const unsigned long long done = record_episode_ends(p, ln.i, o.terminated && ln.valid, !o.legal, rec, episodes, illegal_ends);
    // :86 self.score += score -- the wave's 64 gains go to its slot (G of the return accounting; an illegal move gains 0)
    const uint32_t wave_gain = wave_sum_lane63(ln.valid ? o.gain : 0u);
    const unsigned long long pending = pending_after_step(done, p.auto_reset);
    uint32_t top = 0;
    if (p.highest)
        top = highest(record_cells(rec));                                                        // :97
    if (o.terminated && p.auto_reset != 0)
        reset_record(rec, o, w, tb);

    if (ln.valid) {
        store_board_nt(p.st.boards, ln.i, rec);
        if (STD || p.reward)                                       // :90 / :95
            __builtin_nontemporal_store(o.legal ? static_cast<float>(o.gain) : p.illegal_reward, p.reward + ln.i);
        if (STD || p.terminated)
            __builtin_nontemporal_store(static_cast<uint8_t>(o.terminated ? 1 : 0), p.terminated + ln.i);
        if (p.illegal)
            __builtin_nontemporal_store(static_cast<uint8_t>(o.legal ? 0 : 1), p.illegal + ln.i);
        if (p.highest)
            __builtin_nontemporal_store(static_cast<uint8_t>(top), p.highest + ln.i);
        if (!STD && tail.boards_out)
            store_board(tail.boards_out, ln.i, record_cells(rec));
    }
    flush_episode_counts(counters, episodes, illegal_ends, wave_gain, pending);
    if constexpr (!STD && ACT != 0) {
        if (tail.action_err) // (wave-uniform)
            report_bad_action(tail.action_err, bad.bad && ln.valid, bad.raw, p.board_offset + ln.i);
    }
    if constexpr (HAS_OBS)
        emit_onehot<FULL>(s_recs + (threadIdx.x & ~63u), rec, tail.obs, tail.obs_dtype, ln.i_raw & ~63u, n);
    if (!STD && tail.done_seq)
        signal_done(tail.done_seq, tail.done_value);
}

template <int ACT, bool FULL, bool STD, bool HAS_OBS>
__global__ void __launch_bounds__(kBlock)
step_kernel(uint4 *boards, const void *actions, unsigned long long *ep_counters, uint32_t board_offset, uint32_t seed_lo,
            uint32_t seed_hi, uint32_t t_lo, uint32_t t_hi, uint32_t n, float *reward, const StepTail tail)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    __shared__ uint4 s_recs[HAS_OBS ? kBlock : 1];
    step_body<ACT, FULL, STD, HAS_OBS>(s_tables, s_recs, boards, actions, ep_counters, board_offset, seed_lo, seed_hi, t_lo, t_hi, n,
                                       reward, tail);
}

// The same step with the transaction counter read from DEVICE MEMORY: t = *t_ptr + j.  This is the node of a CACHED
// hipGraph of a k-step launch train (launch_rollout_graph below): the graph's kernel arguments are frozen when it is
// built, so everything that differs between two rollouts over the same buffers -- only t -- comes through memory, written
// by a one-lane set_clock_kernel launch in front of the graph.  Standard configuration only (reward + terminated, no
// optional output).  The s_load of t (uniform address, scalar cache) is in flight together with the board load.
__global__ void __launch_bounds__(64) set_clock_kernel(unsigned long long *t_ptr, unsigned long long value)
{
    if (threadIdx.x == 0)
        *t_ptr = value;
}

template <int ACT, bool FULL>
__global__ void __launch_bounds__(kBlock)
step_graph_kernel(uint4 *boards, const void *actions, unsigned long long *ep_counters, uint32_t board_offset, uint32_t seed_lo,
                  uint32_t seed_hi, const unsigned long long *t_ptr, uint32_t n, uint32_t j, float *reward, const StepTail tail)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const unsigned long long t = *t_ptr + j;
    step_body<ACT, FULL, true, false>(s_tables, nullptr, boards, actions, ep_counters, board_offset, seed_lo, seed_hi,
                                      static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), n, reward, tail);
}

// ------------------------------------------------------------------------- fused rollout
// k steps of the synthetic random policy in ONE launch; the record never leaves registers.
constexpr uint32_t kGainFold = 1024;
__global__ void __launch_bounds__(kBlock) rollout_random_kernel(const StepArgs p)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const Lane ln = lane_of<kBlock, false>(p.n);
    Board rec = load_board(p.st.boards, ln.i);
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    uint64_t t = (static_cast<uint64_t>(p.t_hi) << 32) | p.t_lo; // transaction of the first step
    uint32_t episodes = 0, illegal_ends = 0;
    // this lane's merge scores over the k steps (reduced over the wave once, at the end): one 32-bit add per step, folded
    // into 64 bits every kGainFold steps (a move gains less than the sum of the tiles, < 2^22: 1 024 of them fit 32 bits)
    unsigned long long gained = 0;
    for (uint32_t j0 = 0; j0 < p.k_steps; j0 += kGainFold) {
        const uint32_t j1 = p.k_steps - j0 < kGainFold ? p.k_steps : j0 + kGainFold;
        uint32_t gained32 = 0;
        for (uint32_t j = j0; j < j1; ++j, ++t) {
            const Words w = philox4x32_10(static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), p.board_offset + ln.i, 0u,
                                          p.seed_lo, p.seed_hi);
            const StepOut o = play_record(rec, w.w[3] >> 30, w, p.max_exp, tb);
            gained32 += o.gain;
            record_episode_ends(p, ln.i, o.terminated && ln.valid, !o.legal, rec, episodes, illegal_ends);
            if (o.terminated)
                reset_record(rec, o, w, tb);
        }
        gained += gained32;
    }
    if (ln.valid)
        store_board(p.st.boards, ln.i, rec);
    flush_episode_counts(counters, episodes, illegal_ends, wave_sum64_lane63(ln.valid ? gained : 0ull), 0ull);
}

// ---------------------------------------------------------------- fused rollout with per-step I/O
// The same k steps g2048_rollout performs with k launches, in ONE launch: the record stays in
// registers, each step reads action[j][i] and writes reward[j][i] / terminated[j][i] (stride = elements
// between consecutive steps).  Bit-identical outputs; 6 B of traffic per env-step instead of 38.
//
// The only memory latency on a step's critical path is its action byte, and the only thing a step must not wait
// for is the write acknowledgement of the previous steps' stores.  So the action loads run kPrefetch steps ahead
// of the arithmetic, as a software pipeline in registers: the step loop is unrolled 2 * kPrefetch times over TWO
// register sets -- steps of the first half consume set A and refill set B, the second half consumes B and refills
// A -- so every in-flight action has a fixed register whose old value is dead when the new load is issued (rotating
// registers with moves, or reloading the slot that is being consumed, makes the compiler wait for everything at the
// loop latch).  Step j then waits with s_waitcnt vmcnt(n > 0) for a load issued kPrefetch steps -- thousands of
// cycles -- earlier, and the younger loads and stores stay in flight (RawAction).  The I/O pointers are __restrict__,
// which lets the compiler issue a step's load ahead of the previous steps' stores.
constexpr uint32_t kPrefetch = 4;

template <int ACT>
__global__ void __launch_bounds__(kBlock) rollout_fused_kernel(const StepArgs p, uint64_t stride)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const Lane ln = lane_of<kBlock, false>(p.n);
    const void *__restrict__ actions = p.actions;
    float *__restrict__ reward = p.reward;
    uint8_t *__restrict__ terminated = p.terminated;
    uint8_t *__restrict__ illegal = p.illegal;
    uint8_t *__restrict__ highest_out = p.highest;
    const uint32_t k = p.k_steps;
    // the first kPrefetch actions (register set A) are requested before anything else
    typename RawAction<ACT>::type ahead[kPrefetch];
#pragma unroll
    for (uint32_t q = 0; q < kPrefetch; ++q) {
        ahead[q] = load_action_at<ACT>(actions, static_cast<size_t>(q < k ? q : k - 1u) * stride + ln.i);
        asm volatile("" ::: "memory"); // issue order = consumption order (the scheduler reverses them otherwise, and
                                       // the loop's first wait would then have to cover all of them)
    }
    Board rec = load_board_nt(p.st.boards, ln.i);
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    uint64_t t = (static_cast<uint64_t>(p.t_hi) << 32) | p.t_lo;
    uint32_t episodes = 0, illegal_ends = 0;
    unsigned long long gained = 0; // this lane's merge scores over the k steps: 32-bit adds, folded once per double group
    uint32_t gained32 = 0;
    unsigned long long ended_last = 0; // lanes whose episode the LAST step ended (pending marks when auto_reset == 0)
    // strict actions over k actions: BadAction's fields as two variables (as a struct they change this loop's register allocation)
    bool bad_action = false;
    uint32_t bad_raw = 0;
    // step j with its action; t advances with it
    auto one_step = [&](uint32_t j, uint32_t action_in) {
        const size_t o_idx = static_cast<size_t>(j) * stride + ln.i;
        const Words w = philox4x32_10(static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), p.board_offset + ln.i, 0u,
                                      p.seed_lo, p.seed_hi);
        ++t;
        const uint32_t action = ACT == 0 ? w.w[3] >> 30 : action_in & 3u;
        const StepOut o = play_record(rec, action, w, p.max_exp, tb);
        gained32 += o.gain;
        ended_last = record_episode_ends(p, ln.i, o.terminated && ln.valid, !o.legal, rec, episodes, illegal_ends);
        if (ln.valid) {
            if (reward)
                __builtin_nontemporal_store(o.legal ? static_cast<float>(o.gain) : p.illegal_reward, reward + o_idx);
            if (terminated)
                __builtin_nontemporal_store(static_cast<uint8_t>(o.terminated ? 1 : 0), terminated + o_idx);
            if (illegal)
                __builtin_nontemporal_store(static_cast<uint8_t>(o.legal ? 0 : 1), illegal + o_idx);
            if (highest_out)
                __builtin_nontemporal_store(static_cast<uint8_t>(highest(record_cells(rec))), highest_out + o_idx);
        }
        if (o.terminated && p.auto_reset != 0)
            reset_record(rec, o, w, tb);
    };
    // past the end the last step's action is fetched again and never used (an unconditional load: a conditional one
    // would be waited for where the branches join)
    auto fetch = [&](uint32_t j) { return load_action_at<ACT>(actions, static_cast<size_t>(j < k ? j : k - 1u) * stride + ln.i); };
    // (every action that is played passes through `check` right before its step)
    auto check = [&](typename RawAction<ACT>::type raw) {
        if constexpr (ACT != 0) {
            if (BadAction::outside(raw)) {
                bad_action = true;
                bad_raw = static_cast<uint32_t>(raw);
            }
        }
        return static_cast<uint32_t>(raw);
    };
    typename RawAction<ACT>::type set_b[kPrefetch];
    uint32_t j0 = 0;
    for (; j0 + 2u * kPrefetch <= k; j0 += 2u * kPrefetch) { // whole double groups
#pragma unroll
        for (uint32_t q = 0; q < kPrefetch; ++q) {
            if constexpr (ACT != 0)
                set_b[q] = fetch(j0 + q + kPrefetch);
            one_step(j0 + q, check(ahead[q]));
        }
#pragma unroll
        for (uint32_t q = 0; q < kPrefetch; ++q) {
            if constexpr (ACT != 0)
                ahead[q] = fetch(j0 + q + 2u * kPrefetch);
            one_step(j0 + kPrefetch + q, check(set_b[q]));
        }
        gained += gained32;
        gained32 = 0;
    }
    // the last k % (2 * kPrefetch) steps: the first kPrefetch of them have their actions in flight already
#pragma unroll
    for (uint32_t q = 0; q < kPrefetch; ++q)
        if (j0 + q < k)
            one_step(j0 + q, check(ahead[q]));
    for (uint32_t j = j0 + kPrefetch; j < k; ++j)
        one_step(j, check(fetch(j)));
    gained += gained32; // (at most 2 * kPrefetch - 1 tail steps)
    if (ln.valid)
        store_board_nt(p.st.boards, ln.i, rec);
    flush_episode_counts(counters, episodes, illegal_ends, wave_sum64_lane63(ln.valid ? gained : 0ull),
                         pending_after_step(ended_last, p.auto_reset));
    if constexpr (ACT != 0) {
        if (p.action_err)
            report_bad_action(p.action_err, bad_action && ln.valid, bad_raw, p.board_offset + ln.i);
    }
}

// ------------------------------------------------------------------------- numpy-RNG mode
// Same step / reset / add_tile, drawing from each board's own PCG64 exactly as numpy would
// (g2048_pcg64.h).  RNG state: five coalesced 8-byte planes.
__device__ __forceinline__ Pcg64 load_rng(const uint64_t *planes, uint32_t n, uint32_t i)
{
    return Pcg64{planes[i], planes[n + i], planes[2ull * n + i], planes[3ull * n + i], planes[4ull * n + i]};
}

__device__ __forceinline__ void store_rng(uint64_t *planes, uint32_t n, uint32_t i, const Pcg64 &r)
{
    planes[i] = r.state_lo;
    planes[n + i] = r.state_hi;
    planes[4ull * n + i] = r.buf; // inc never changes
}

// ... except where it is made: seeding
__device__ __forceinline__ void store_rng_all(uint64_t *planes, uint32_t n, uint32_t i, const Pcg64 &r)
{
    planes[i] = r.state_lo;
    planes[n + i] = r.state_hi;
    planes[2ull * n + i] = r.inc_lo;
    planes[3ull * n + i] = r.inc_hi;
    planes[4ull * n + i] = r.buf;
}

// Game2048Env.step + the caller's `if terminated: env.reset()` in ONE launch.  A spawn in this mode is ~1 000 VALU
// instructions (15 accepted draws of the Fisher-Yates shuffle over 32-bit halves of a 128-bit LCG, in lockstep per
// wavefront), and a reset is two of them: run in-lane it would be executed by 99 % of the wavefronts for the 7 % of the
// boards that need it.  Until round 6 the finished boards were listed per wavefront and reset by a SECOND, compacted
// kernel (19 us behind a 42.6 us step at 2^20 boards: two waves per SIMD, each a serial chain of 128-bit multiplies).
// Now the compaction happens inside the launch, per 512-lane block: a lane whose episode ended hands its generator over
// through LDS instead of storing it (slot = the block's running count + its rank among the wavefront's finished lanes),
// and behind ONE barrier the block's first `total` lanes -- under a random policy ~36 of 512: part of one wavefront,
// the other seven retire -- each reset one listed board and store its fresh record and generator.  The reset work of
// a block overlaps the step work of the other blocks on the CU.
// (512 lanes: 45.0-46.1 us per step at 2^20 boards against 48.2 / 48.7 / 48.4 for 256 / 768 / 1 024, one box,
//  profiles/r06_d_numpy_block_ab.txt; forcing 8 waves per SIMD -- 64 VGPRs, five dwords spilled -- changes nothing.
//  Measured "no", same round: a software pipeline over 2 / 4 / 8 tiles per block with the next tile's records and generators
//  prefetched into registers and a ninth, reset-only wavefront: 65 / 61 / 59 us -- 89 VGPRs leave four stepping wavefronts
//  per SIMD and the serial 128-bit multiply chains need six to fill the VALU, profiles/r06_g_numpy_tiles_ab.txt; starting
//  the odd blocks 3.4 us late to pull the load / compute / store phases of co-resident blocks apart: +10 us,
//  profiles/r06_h_numpy_stagger_ab.txt.  What does help is not touching memory per step at all: rollout_fused_numpy_kernel.)
constexpr uint32_t kNumpyBlock = 512;
static_assert(kNumpyBlock == kSlotBlockLanes, "the slot array is sized for whole blocks of this kernel");

template <int ACT>
__global__ void __launch_bounds__(kNumpyBlock) step_numpy_kernel(const StepArgs p)
{
    __shared__ uint64_t s_rng[5][kNumpyBlock]; // the generators handed over (plane-major: conflict-free), 20 KiB
    __shared__ uint16_t s_who[kNumpyBlock];    // ... whose they are (lane index in the block) ...
    __shared__ uint8_t s_first[kNumpyBlock];   // ... and the first tile of the reset where it is drawn already: cell | four << 4, else 0xff
    __shared__ uint32_t s_count;
    if (threadIdx.x == 0u)
        s_count = 0u;
    const Lane ln = lane_of<kNumpyBlock, false>(p.n);
    Board rec = load_board(p.st.boards, ln.i);
    Pcg64 rng = load_rng(p.st.rng, p.n, ln.i);
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    uint32_t action;
    if constexpr (ACT == 0)
        action = philox4x32_10(p.t_lo, p.t_hi, p.board_offset + ln.i, 0u, p.seed_lo, p.seed_hi).w[3] >> 30;
    else {
        BadAction bad;
        action = bad.note_only(load_action_at<ACT>(p.actions, ln.i));
        if (p.action_err) // strict actions (wave-uniform)
            report_bad_action(p.action_err, bad.bad && ln.valid, bad.raw, p.board_offset + ln.i);
    }
    if (p.auto_reset != 0u)
        __syncthreads(); // s_count = 0 is visible before the first hand-over (placed here: the loads above are in flight)

    // rec: the terminal record where the episode ended.  A lane whose move is illegal draws the first tile of its reset here
    const NumpyStepOut o = play_record_numpy(rec, action, rng, p.max_exp, p.auto_reset != 0u);
    const uint32_t wave_gain = wave_sum_lane63(ln.valid ? o.gain : 0u);         // :86

    const bool fin = o.terminated && ln.valid;
    const bool hand_over = fin && p.auto_reset != 0u;
    if (ln.valid) {
        if (!hand_over) { // (a board that is reset below is stored there, once)
            store_board(p.st.boards, ln.i, rec);
            store_rng(p.st.rng, p.n, ln.i, rng);
        }
        if (p.reward)
            p.reward[ln.i] = o.legal ? static_cast<float>(o.gain) : p.illegal_reward;  // :90 / :95
        if (p.terminated)
            p.terminated[ln.i] = o.terminated ? 1 : 0;
        if (p.illegal)
            p.illegal[ln.i] = o.legal ? 0 : 1;
        if (p.highest)
            p.highest[ln.i] = static_cast<uint8_t>(o.top);
    }
    uint32_t episodes = 0, illegal_ends = 0;
    const unsigned long long ended = record_episode_ends(p, ln.i, fin, !o.legal, rec, episodes, illegal_ends);
    flush_episode_counts(counters, episodes, illegal_ends, wave_gain, pending_after_step(ended, p.auto_reset));
    if (p.auto_reset == 0u) // (kernel-uniform)
        return;
    // ---- `if terminated: env.reset()` (game2048_env.py:102-111), compacted over the block
    const unsigned long long done = __builtin_amdgcn_ballot_w64(hand_over);
    if (done != 0ull) { // (wave-uniform)
        uint32_t base = 0;
        if ((threadIdx.x & 63u) == 0u)
            base = atomicAdd(&s_count, static_cast<uint32_t>(__popcll(done)));
        base = __builtin_amdgcn_readfirstlane(base);
        if (hand_over) {
            const uint32_t e = base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(done >> 32),
                                                                __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(done), 0u));
            s_who[e] = static_cast<uint16_t>(threadIdx.x);
            s_first[e] = o.have_first ? static_cast<uint8_t>(o.first_cell | (o.first_four ? 16u : 0u)) : static_cast<uint8_t>(0xffu);
            s_rng[0][e] = rng.state_lo;
            s_rng[1][e] = rng.state_hi;
            s_rng[2][e] = rng.inc_lo;
            s_rng[3][e] = rng.inc_hi;
            s_rng[4][e] = rng.buf;
        }
    }
    __syncthreads();
    const uint32_t total = s_count;
    if ((threadIdx.x & ~63u) >= total) // (whole wavefronts stay or go: finish_record_numpy votes)
        return;
    const bool mine = threadIdx.x < total;
    const uint32_t e = mine ? threadIdx.x : 0u;
    const uint32_t j = blockIdx.x * kNumpyBlock + s_who[e];
    const uint32_t first = s_first[e];
    Pcg64 r2{s_rng[0][e], s_rng[1][e], s_rng[2][e], s_rng[3][e], s_rng[4][e]};
    const Board fresh = finish_record_numpy(r2, first != 0xffu || !mine, first & 15u, (first & 16u) != 0u);
    if (mine) {
        store_board(p.st.boards, j, fresh);
        store_rng(p.st.rng, p.n, j, r2);
    }
}

// ---- k steps of numpy-RNG mode in ONE launch, record and generator in registers (g2048_rollout_fused / _random)
// A reset in this mode is two ~1 000-instruction spawns that only the 7 % of the lanes whose episode ended need: the
// per-step kernel above compacts them over the block, which a kernel that keeps its boards in registers cannot do without
// shipping generators through LDS twice per step.  Instead the lanes of a wavefront are allowed to DRIFT IN TIME: every
// trip of the loop is one lockstep spawn, and each lane spends it on what IT needs next --
//   * a lane that is stepping plays its own step j (its own row of the [k][n] buffers) and spawns that step's tile;
//   * a lane whose move was illegal spawns nothing in its step (game2048_env.py:91-95), so it draws the FIRST tile of its
//     reset in the same trip, and the second one in the next trip while its neighbours play their next step;
//   * a lane whose episode ended on a legal move (no moves left / max_tile) spends the next two trips on its reset;
// and the loop ends when every lane has played k steps and finished its resets.  A board's generator is consumed in exactly
// the reference's order (step spawn, then the reset's two), whatever its neighbours do.  Under a random policy a lane
// resets ~0.07 times per step, nearly always after an illegal move: ~1.1 trips per step instead of the 3 an in-lane reset
// would cost every wavefront.  The price is I/O that is no longer coalesced once the lanes have drifted apart (each lane
// reads / writes ITS row j): 6 B per env-step through partially written lines, which the L2 and the Infinity Cache merge.
template <int ACT>
__global__ void __launch_bounds__(kBlock) rollout_fused_numpy_kernel(const StepArgs p, uint64_t stride)
{
    const Lane ln = lane_of<kBlock, false>(p.n);
    Board rec = load_board(p.st.boards, ln.i);
    Pcg64 rng = load_rng(p.st.rng, p.n, ln.i);
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    const uint64_t t0 = (static_cast<uint64_t>(p.t_hi) << 32) | p.t_lo; // transaction of this lane's step 0
    const uint32_t k = p.k_steps;
    uint32_t j = 0;        // the step this lane plays next
    uint32_t phase = 0;    // 0: stepping; 1: reset pending, no tile drawn yet; 2: reset pending, first tile drawn
    Board fresh{{0u, 0u, 0u, 0u}};
    uint32_t fresh_fours = 0;
    uint32_t episodes = 0, illegal_ends = 0, gained32 = 0;
    unsigned long long gained = 0;
    bool last_ended = false; // this lane's step k - 1 ended its episode (the pending mark when auto_reset == 0)
    bool bad_action = false; // (BadAction spelled out: see rollout_fused_kernel)
    uint32_t bad_raw = 0;
    for (;;) {
        const bool stepping = phase == 0u && j < k;
        if (!g2048_any(stepping || phase != 0u)) // (wave-uniform)
            break;
        // ---- the step's move (lanes that are stepping)
        uint32_t gain = 0;
        bool legal = false;
        Board cells = record_cells(rec);
        const size_t io_idx = static_cast<size_t>(j < k ? j : 0u) * stride + ln.i;
        if (stepping) {
            uint32_t action;
            if constexpr (ACT == 0) {
                const uint64_t t = t0 + j;
                action = philox4x32_10(static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), p.board_offset + ln.i, 0u, p.seed_lo,
                                       p.seed_hi).w[3] >> 30;
            } else {
                const typename RawAction<ACT>::type v = load_action_at<ACT>(p.actions, io_idx);
                typedef typename std::make_unsigned<typename RawAction<ACT>::type>::type U;
                if (static_cast<U>(v) > static_cast<U>(3)) { // = BadAction::outside(v), which costs this loop its registers' order
                    bad_action = true;
                    bad_raw = static_cast<uint32_t>(v);
                }
                action = static_cast<uint32_t>(v) & 3u;
            }
            legal = move(cells, action, gain);                                  // :85
        }
        // ---- the trip's ONE lockstep spawn: the step's tile, or a tile of the lane's reset
        const bool early = stepping && !legal && p.auto_reset != 0u;            // illegal move: first reset tile now
        const bool spawn = (stepping && legal) || early || phase != 0u;
        Board target = (stepping && legal) ? cells : (phase == 2u ? fresh : Board{{0u, 0u, 0u, 0u}});
        bool four = false;
        if (spawn)
            four = add_tile_numpy(target, rng);                                 // :88 / :108 / :109
        // ---- what the spawn was for
        bool fin = false;
        if (stepping) {
            bool end = false;
            if (legal) {
                cells = target;
                end = is_end(cells, p.max_exp);                                 // :89
            }
            const bool terminated = legal ? end : true;                         // :89, :94
            record_update(rec, cells, (legal && four) ? 0x80u : 0u);            // a spawned 4: deficit += 4
            gained32 += gain;                                                   // :86
            if (ln.valid) {
                if (p.reward)
                    __builtin_nontemporal_store(legal ? static_cast<float>(gain) : p.illegal_reward, p.reward + io_idx);
                if (p.terminated)
                    __builtin_nontemporal_store(static_cast<uint8_t>(terminated ? 1 : 0), p.terminated + io_idx);
                if (p.illegal)
                    __builtin_nontemporal_store(static_cast<uint8_t>(legal ? 0 : 1), p.illegal + io_idx);
                if (p.highest)
                    __builtin_nontemporal_store(static_cast<uint8_t>(highest(cells)), p.highest + io_idx);
            }
            fin = terminated && ln.valid;
            if (j + 1u == k)
                last_ended = fin;
            ++j;
            if (terminated && p.auto_reset != 0u) {                             // the caller's `if terminated: env.reset()`
                phase = early ? 2u : 1u;
                fresh = target;                                                 // (early: the empty board + its first tile)
                fresh_fours = (early && four) ? 1u : 0u;
            }
        } else if (phase == 1u) {
            fresh = target;
            fresh_fours = four ? 1u : 0u;
            phase = 2u;
        } else if (phase == 2u) {
            fresh_fours += four ? 1u : 0u;
            rec = target;                                                       // :104-109: score 0, so deficit = 4 per spawned 4
            rec.r[2] |= fresh_fours == 1u ? 0x80u : (fresh_fours == 2u ? 0x2000u : 0u);
            phase = 0u;
        }
        // episode ends of this trip (terminal record first: rec still holds it -- a reset only lands two trips later)
        (void)record_episode_ends(p, ln.i, fin, !legal, rec, episodes, illegal_ends);
        if ((gained32 >> 30) != 0u) { // (a lane gains < 2^18 per step: folded long before it could wrap)
            gained += gained32;
            gained32 = 0;
        }
    }
    gained += gained32;
    if (ln.valid) {
        store_board(p.st.boards, ln.i, rec);
        store_rng(p.st.rng, p.n, ln.i, rng);
    }
    const unsigned long long ended_last = __builtin_amdgcn_ballot_w64(last_ended);
    flush_episode_counts(counters, episodes, illegal_ends, wave_sum64_lane63(ln.valid ? gained : 0ull),
                         pending_after_step(ended_last, p.auto_reset));
    if constexpr (ACT != 0) {
        if (p.action_err)
            report_bad_action(p.action_err, bad_action && ln.valid, bad_raw, p.board_offset + ln.i);
    }
}

// numpy's PCG64(SeedSequence(base_seed + global board index)) for every board, computed on the device.
__global__ void __launch_bounds__(kBlock) seed_numpy_kernel(uint64_t *planes, uint32_t n, uint64_t first_seed)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    store_rng_all(planes, n, i, pcg64_from_seed(first_seed + i));
}

// Return accounting of an explicit reset (g2048_reset; whole wavefronts): see adjust_slot.
__device__ __forceinline__ void account_reset(const StepArgs &p, uint32_t i_raw, uint32_t i, bool doit)
{
    const bool was_pending = is_pending(p.st.ep_counters, i_raw);
    int32_t delta = 0;
    if (doit && !was_pending) // an episode that is still running is abandoned: its score leaves the books
        delta = -static_cast<int32_t>(record_score(load_board(p.st.boards, i)));
    adjust_slot(p.st.ep_counters, i_raw, delta, doit);
}

__global__ void __launch_bounds__(kBlock) reset_numpy_kernel(const StepArgs p, const uint8_t *mask)
{
    const Lane ln = lane_of<kBlock, false>(p.n);
    const bool doit = ln.valid && !(mask && mask[ln.i] == 0);
    account_reset(p, ln.i_raw, ln.i, doit);
    if (!doit)
        return;
    Pcg64 rng = load_rng(p.st.rng, p.n, ln.i);
    const Board fresh = fresh_record_numpy(rng); // game2048_env.py:104-109
    store_rng(p.st.rng, p.n, ln.i, rng);
    store_board(p.st.boards, ln.i, fresh);
}

__global__ void __launch_bounds__(kBlock) add_tile_numpy_kernel(const StepArgs p)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= p.n)
        return;
    const Board raw = load_board(p.st.boards, i);
    Board bd = record_cells(raw);
    if (count_empty(bd) == 0)
        return;
    Pcg64 rng = load_rng(p.st.rng, p.n, i);
    const bool four = add_tile_numpy(bd, rng);
    store_rng(p.st.rng, p.n, i, rng);
    Board rec = raw;
    record_update(rec, bd, four ? 0x80u : 0u); // a spawned 4 raises the potential without scoring: deficit += 4
    store_board(p.st.boards, i, rec);
}

// ---------------------------------------------------------------------------------- reset
// Game2048Env.reset for every (masked) board (game2048_env.py:102-111).
__global__ void __launch_bounds__(kBlock) reset_kernel(const StepArgs p, uint32_t first_slot, const uint8_t *mask)
{
    const Lane ln = lane_of<kBlock, false>(p.n);
    const bool doit = ln.valid && !(mask && mask[ln.i] == 0);
    account_reset(p, ln.i_raw, ln.i, doit);
    if (!doit)
        return;
    const uint32_t b = p.board_offset + ln.i;
    const Words w = philox4x32_10(p.t_lo, p.t_hi, b, first_slot >> 2, p.seed_lo, p.seed_hi);
    const uint32_t s = first_slot & 3u;
    const uint32_t w1 = select_word(w, s);
    uint32_t w2;
    if (s == 3u) // the second spawn lives in the next block of this transaction
        w2 = philox4x32_10(p.t_lo, p.t_hi, b, (first_slot >> 2) + 1u, p.seed_lo, p.seed_hi).w[0];
    else
        w2 = select_word(w, s + 1u);
    store_board(p.st.boards, ln.i, fresh_record(w1, w2)); // score 0 (:105) is part of the record
}

// ------------------------------------------------------------------------- game primitives
// Game2048Env.move alone (game2048_env.py:194-241): no spawn, no score, no clock.
template <int ACT>
__global__ void __launch_bounds__(kBlock) move_kernel(uint4 *boards, uint32_t n, const void *actions, uint32_t trial,
                                                      int32_t *score_out, uint8_t *legal_out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const Board raw = load_board(boards, i);
    Board bd = record_cells(raw);
    uint32_t gain;
    const bool legal = move(bd, action_bits(load_action_at<ACT>(actions, i)), gain);
    if (score_out)
        score_out[i] = legal ? static_cast<int32_t>(gain) : 0;
    if (legal_out)
        legal_out[i] = legal ? 1 : 0;
    if (!trial && legal)
        store_board(boards, i, make_record(bd, record_score(raw))); // self.score is not touched by move()
}

// Game2048Env.isend (game2048_env.py:262-280) and highest (:190-192).
__global__ void __launch_bounds__(kBlock) query_kernel(const uint4 *boards, uint32_t n, uint32_t max_exp,
                                                       uint8_t *isend_out, uint8_t *highest_out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const Board bd = record_cells(load_board(boards, i));
    if (isend_out)
        isend_out[i] = is_end(bd, max_exp) ? 1 : 0;
    if (highest_out)
        highest_out[i] = static_cast<uint8_t>(highest(bd));
}

// The four trial moves of isend (game2048_env.py:273-280) as a mask: bit d = move d changes the board.
__global__ void __launch_bounds__(kBlock) legal_mask_kernel(const uint4 *boards, uint32_t n, uint8_t *mask_out)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const Board cells = record_cells(load_board(boards, i));
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t d = 0; d < 4u; ++d) {
        Board trial = cells;                                   // trial=True: the board itself is left alone (:224,:236)
        uint32_t gain;
        if (move_sel(trial, tb.move_sel(d), gain))
            mask |= 1u << d;
    }
    mask_out[i] = static_cast<uint8_t>(mask);
}

// Game2048Env.add_tile (game2048_env.py:166-176) from spawn slot `slot` of transaction t.
__global__ void __launch_bounds__(kBlock) add_tile_kernel(const StepArgs p, uint32_t slot)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= p.n)
        return;
    const Board raw = load_board(p.st.boards, i);
    Board bd = record_cells(raw);
    if (count_empty(bd) == 0) // the reference asserts here (:176)
        return;
    const Words w = philox4x32_10(p.t_lo, p.t_hi, p.board_offset + i, slot >> 2, p.seed_lo, p.seed_hi);
    add_tile(bd, select_word(w, slot & 3u));
    store_board(p.st.boards, i, make_record(bd, record_score(raw)));
}

// The cells of a loaded 16-byte input row.  PLAIN: plain exponents, taken mod 32; otherwise an engine record, whose
// deficit bits are dropped.
template <bool PLAIN> __device__ __forceinline__ Board input_cells(const Board &in)
{
    if constexpr (PLAIN)
        return Board{{in.r[0] & kCellBits, in.r[1] & kCellBits, in.r[2] & kCellBits, in.r[3] & kCellBits}};
    else
        return record_cells(in);
}

// ------------------------------------------------------------- records <-> plain boards / scores
// get_board / set_board (game2048_env.py:282-288) and self.score for the whole batch.
__global__ void __launch_bounds__(kBlock) export_boards_kernel(const uint4 *records, uint32_t n, uint4 *cells_out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n)
        store_board(cells_out, i, record_cells(load_board(records, i)));
}

__global__ void __launch_bounds__(kBlock) import_boards_kernel(uint4 *records, uint32_t n, const uint4 *cells_in)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const Board cells = input_cells<true>(load_board(cells_in, i));
    store_board(records, i, make_record(cells, record_score(load_board(records, i)))); // score untouched (:286-288)
}

__global__ void __launch_bounds__(kBlock) export_scores_kernel(const uint4 *records, uint32_t n, int32_t *scores_out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n)
        scores_out[i] = static_cast<int32_t>(record_score(load_board(records, i)));
}

__global__ void __launch_bounds__(kBlock) import_scores_kernel(uint4 *records, uint32_t n, const int32_t *scores_in,
                                                               unsigned long long *ep_counters)
{
    const Lane ln = lane_of<kBlock, false>(n);
    const Board raw = load_board(records, ln.i);
    const uint32_t score = static_cast<uint32_t>(scores_in[ln.i]) & kScoreMask;
    // return accounting: the live score of a running episode changes by (new - old); a board whose episode has ended
    // keeps its place among the finished ones
    const bool live = ln.valid && !is_pending(ep_counters, ln.i_raw);
    adjust_slot(ep_counters, ln.i_raw, live ? static_cast<int32_t>(score) - static_cast<int32_t>(record_score(raw)) : 0, false);
    if (ln.valid)
        store_board(records, ln.i, make_record(record_cells(raw), score));
}

// g2048_seed: forget the finished episodes (game2048_env.py:103 restarts the stream).  Every slot restarts with
// G = the scores its 64 boards hold right now (so "G - live scores" = 0: no finished episode) and no pending marks.
__global__ void __launch_bounds__(kBlock) clear_stats_kernel(const DeviceState st, uint32_t n)
{
    const uint32_t i_raw = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i_raw < n;
    uint32_t score = 0;
    if (valid) {
        if (st.last_record)
            st.last_record[i_raw] = make_uint4(0u, 0u, 0u, 0u);
        score = record_score(load_board(st.boards, i_raw));
    }
    const uint32_t total = wave_sum_lane63(score); // <= 64 * (2^24 - 1)
    if ((threadIdx.x & 63u) == 63u) {
        uint32_t *slot = slot_of(st.ep_counters, i_raw >> 6);
        slot_set(slot, kSlotEpisodes, 0ull);
        slot_set(slot, kSlotIllegal, 0ull);
        slot_set(slot, kSlotGain, total);
        slot_set(slot, kSlotPending, 0ull);
    }
}

// final score of each board's most recent finished episode (0 before the first one)
__global__ void __launch_bounds__(kBlock) export_last_scores_kernel(const uint4 *last_record, uint32_t n, int32_t *out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n)
        out[i] = static_cast<int32_t>(record_score(load_board(last_record, i)));
}

// ------------------------------------------------------------------------ synthetic policy
__global__ void __launch_bounds__(kBlock) fill_actions_kernel(uint8_t *out, uint32_t n, uint32_t board_offset,
                                                              uint32_t seed_lo, uint32_t seed_hi, uint64_t t_first,
                                                              uint32_t k_steps)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t j = blockIdx.y;
    if (i >= n || j >= k_steps)
        return;
    const uint64_t t = t_first + j;
    const Words w = philox4x32_10(static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32), board_offset + i, 0u,
                                  seed_lo, seed_hi);
    out[static_cast<size_t>(j) * n + i] = static_cast<uint8_t>(w.w[3] >> 30);
}

// ---------------------------------------------------------------------------------- onehot
// stack() (game2048_env.py:17-32): board record -> (16,4,4), channel c = (exponent == c).  One lane writes
// one 16-byte chunk of the output, so every store is a coalesced dwordx4:
//   u8 : chunk = one channel (16 cells)            16 chunks / board
//   f16: chunk = half a channel (8 cells)          32 chunks / board
//   f32: chunk = one row of one channel (4 cells)  64 chunks / board
template <int OBS>
__global__ void __launch_bounds__(kBlock) onehot_kernel(const uint4 *__restrict__ boards, uint64_t chunks,
                                                        uint4 *__restrict__ out)
{
    const uint64_t g = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= chunks)
        return;
    const uint32_t *cells = reinterpret_cast<const uint32_t *>(boards);
    if constexpr (OBS == 0) {
        const uint64_t board = g >> 4;
        const uint32_t splat = static_cast<uint32_t>(g & 15u) * 0x01010101u;
        const uint4 v = boards[board];
        store_chunk_nt(out, g, z80(v.x ^ splat) >> 7, z80(v.y ^ splat) >> 7, z80((v.z & kCellBits) ^ splat) >> 7,
                       z80((v.w & kCellBits) ^ splat) >> 7);
    } else if constexpr (OBS == 1) {
        const uint64_t board = g >> 5;
        const uint32_t c = static_cast<uint32_t>(g >> 1) & 15u, half = static_cast<uint32_t>(g) & 1u;
        const uint32_t r0 = cells[board * 4 + half * 2] & kCellBits, r1 = cells[board * 4 + half * 2 + 1] & kCellBits;
        uint32_t h[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            h[k] = (((r0 >> (8 * k)) & 0xffu) == c) ? 0x3c00u : 0u; // fp16 1.0
            h[4 + k] = (((r1 >> (8 * k)) & 0xffu) == c) ? 0x3c00u : 0u;
        }
        store_chunk_nt(out, g, h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    } else {
        const uint64_t board = g >> 6;
        const uint32_t c = static_cast<uint32_t>(g >> 2) & 15u, row = static_cast<uint32_t>(g) & 3u;
        const uint32_t r = cells[board * 4 + row] & kCellBits;
        uint32_t f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            f[k] = (((r >> (8 * k)) & 0xffu) == c) ? 0x3f800000u : 0u; // fp32 1.0
        store_chunk_nt(out, g, f[0], f[1], f[2], f[3]);
    }
}

// ---------------------------------------------------------------------------- afterstates
// The four trial moves of legal_mask_kernel, keeping what they produce (g2048_afterstates): per board the afterstate of
// every direction (4 x 16 B), the four merge scores (16 B), the legality mask (1 B) and, when asked, stack() of the four
// afterstates (4 x 256 / 512 / 1 024 B).  One board per lane, move_sel with the LDS selector rows as in step_body; an
// illegal direction leaves the board unchanged with gain 0 (:224,:236-239).  Nothing is written back: the records, the
// clock, the episode slots and the randomness are not touched.  PLAIN: the input is plain exponents (taken mod 32)
// instead of engine records (whose deficit bits are dropped); OBS: o.obs is set (the one-hot code is compiled only into
// the kernels that write it: it doubles the VGPR count).
//
// Stores.  The scores of consecutive lanes are consecutive 16-byte rows and the masks consecutive bytes: coalesced as
// they are.  The afterstates are 64 B per lane: the wave's 256 afterstates are parked in LDS (4 KiB, afterstate
// 4 * lane + d) and written as four fully coalesced 16-byte streaming stores (store s, lane l: chunk s * 64 + l), the
// scheme of emit_onehot -- 2.7x faster at 2^20 boards and 3.4x at 2^24 than each lane storing its own four chunks at a
// 64-B lane stride (profiles/r07_afterstates_probe.txt).  The observation of the same 256 afterstates is written from
// LDS too: emit_onehot_as over four quarters of 64.
// Occupancy with an observation is capped at 2 workgroups per CU like the other observation writers (kObsOccupancyPad):
// here the static LDS is 18 KiB, so the pad that makes a workgroup own 64 KiB is 46 KiB -- below the 48 KiB that needs
// no opt-in.
constexpr uint32_t kAfterstateStaticLds = sizeof(WaveTables) * (kBlock / 64) + sizeof(Cells16) * kBlock * 4u;
constexpr uint32_t kAfterstateObsPad = 64u * 1024u - kAfterstateStaticLds;
static_assert(kAfterstateObsPad <= 48u * 1024u, "afterstate occupancy pad needs the dynamic-LDS opt-in");

template <bool PLAIN, bool OBS>
__global__ void __launch_bounds__(kBlock) afterstates_kernel(const uint4 *__restrict__ boards, uint32_t n, const AfterstateOut o)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    __shared__ Cells16 s_after[kBlock * 4];
    const uint2 piece = load_tables_piece();
    const uint32_t i_raw = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i_raw < n;
    const uint32_t i = valid ? i_raw : n - 1u; // lanes past the end move a copy of the last board and store nothing
    const Board in = load_board_nt(boards, i);
    const LdsTables tb = stage_tables(s_tables, piece);
    const Board cells = input_cells<PLAIN>(in);
    Board after[4];
    uint32_t gain[4], mask = 0;
#pragma unroll
    for (uint32_t d = 0; d < 4u; ++d) {
        after[d] = cells;
        if (move_sel(after[d], tb.move_sel(d), gain[d])) // false: after[d] == cells, gain 0
            mask |= 1u << d;
    }
    if (valid && o.legal)
        o.legal[i] = static_cast<uint8_t>(mask);
    if (valid && o.score)
        store_chunk_nt(o.score, i, gain[0], gain[1], gain[2], gain[3]);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_first = __builtin_amdgcn_readfirstlane(i_raw & ~63u);
    const uint32_t n_after = wave_first < n ? 4u * (n - wave_first < 64u ? n - wave_first : 64u) : 0u; // this wave's
    Cells16 *recs = s_after + (threadIdx.x & ~63u) * 4u;
#pragma unroll
    for (uint32_t d = 0; d < 4u; ++d) {
        Cells16 &r = recs[lane * 4u + d];
        r.r[0] = after[d].r[0], r.r[1] = after[d].r[1], r.r[2] = after[d].r[2], r.r[3] = after[d].r[3];
    }
    // same-wave LDS accesses execute in program order; the fences keep the compiler from reordering them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (o.boards) {
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint32_t j = s * 64u + lane;
            if (j < n_after)
                store_chunk_nt(o.boards, static_cast<uint64_t>(wave_first) * 4u + j, recs[j].r[0], recs[j].r[1],
                               recs[j].r[2], recs[j].r[3]);
        }
    }
    if (OBS) {
        // quarter q = afterstates 64q .. 64q + 63 of the wave: one emit_onehot piece of 16 / 32 / 64 KiB
        for (uint32_t q = 0; q < 4u && 64u * q < n_after; ++q) {
            const uint32_t n_q = n_after - 64u * q < 64u ? n_after - 64u * q : 64u;
            uint4 *out = static_cast<uint4 *>(o.obs) + ((static_cast<uint64_t>(wave_first) * 4u + 64u * q) << (4u + o.obs_dtype));
            if (o.obs_dtype == 0u)
                emit_onehot_as<0, false>(recs + 64u * q, out, lane, n_q);
            else if (o.obs_dtype == 1u)
                emit_onehot_as<1, false>(recs + 64u * q, out, lane, n_q);
            else
                emit_onehot_as<2, false>(recs + 64u * q, out, lane, n_q);
        }
    }
}

// ---------------------------------------------------------------------------- expectimax
// g2048_expectimax: the depth-D search of g2048_device.h ("expectimax search") for every board.  A board is a group of G
// lanes, K = G / 4 per root direction d; lane `sub` of direction d sums the chance items sub, sub + K, ... of that
// direction's afterstate (chance_partial), the K partial sums meet in an xor-shuffle tree and the four directions pick
// the action with one more max over the group.  Depth 1 (about 2E leaves per direction) takes G = 4; depths 2 and 3
// (about 4 * 2E times as many per level) spread one board over a whole wave, G = 64, so 2^12 boards are already 4 096
// waves.  The sums are integers: every split gives the same bits as search_root on the host.  Lanes stride over the
// boards when n * G exceeds the grid cap (kSearchMaxLanes).  Nothing is written back: no record, clock, episode slot or
// randomness is touched.  PLAIN: plain exponents (mod 32) instead of engine records.
constexpr uint64_t kSearchMaxLanes = 1ull << 24;

// Lane j of a board's group of G: lane `sub` of the K = G / 4 that share root direction d.  The groups take the boards
// first, first + stride, ...; a group's G lanes hold the same board index, so they leave that loop together and every
// shuffle stays inside live groups.
template <uint32_t G> struct LaneGroup {
    static constexpr uint32_t K = G / 4u;
    const uint32_t j = threadIdx.x % G, d = j / K, sub = j % K;
    const uint32_t stride = gridDim.x * (kBlock / G);
    const uint64_t first = (static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x) / G;
};

// The largest key of the group's four directions, in every lane (the K lanes of a direction hold equal keys)
template <class KEY> __device__ __forceinline__ KEY group_best_key(KEY key, uint32_t K)
{
    KEY other = __shfl_xor(key, K);
    key = other > key ? other : key;
    other = __shfl_xor(key, 2u * K);
    return other > key ? other : key;
}

template <int D, bool PLAIN>
__global__ void __launch_bounds__(kBlock) expectimax_kernel(const uint4 *__restrict__ boards, uint32_t n, const SearchArgs a)
{
    constexpr uint32_t G = D == 1 ? 4u : 64u, K = G / 4u;
    __shared__ WaveTables s_tables[kBlock / 64];
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const SearchWeights w{a.base, a.w_empty, a.w_merge, a.w_mono};
    const LaneGroup<G> grp;
    const uint32_t j = grp.j, d = grp.d, sub = grp.sub;
    for (uint64_t i = grp.first; i < n; i += grp.stride) {
        const Board in = load_board(boards, static_cast<uint32_t>(i));
        const Board cells = input_cells<PLAIN>(in);
        Board after = cells;
        uint32_t gain;
        const bool legal = move_sel(after, tb.move_sel(d), gain);
        uint64_t part = 0;
        if (legal)
            part = chance_partial<D>(after, sub, K, w, tb);
#pragma unroll
        for (uint32_t o = K / 2u; o > 0u; o >>= 1)
            part += __shfl_xor(part, o);
        const int32_t value = legal ? static_cast<int32_t>(part / (10u * count_empty(after))) : -1;
        const uint32_t key = group_best_key(root_key<uint32_t>(value, d), K);
        if (sub == 0u && a.value)
            a.value[i * 4u + d] = value;
        if (j == 0u && a.action)
            a.action[i] = static_cast<uint8_t>(root_key_action(key));
    }
}

// ---------------------------------------------------------------------------- Monte-Carlo rollout search
// g2048_mc_search: the rollout search of g2048_device.h ("Monte-Carlo rollout search") for every board.  A board is a
// group of G lanes, K = G / 4 per root direction d; lane `sub` of direction d runs the playouts sub, sub + K, ... < R of
// that direction.  Playouts end hundreds of moves apart, so the lanes of a wave do not run them in step: the wave runs
// ONE flat loop of mc_trip, in which every lane is at its own playout, move and candidate direction -- a lane whose
// playout ended begins its next one on the following trip -- and leaves it when no lane has a playout left (one ballot).
// The board stays in registers, the selector rows come from LDS; memory sees one 16-byte load per board and the
// outputs.  The result is a sum of pure functions of (i, d, r), so this schedule gives the bits of mc_root on the host.
// G = 64 (one wave per board) when R >= kMcWaveRollouts, else G = 16, which keeps the lanes of a direction busy at small
// R.  Lanes stride over the boards when n * G exceeds the grid cap (kSearchMaxLanes); PLAIN as in expectimax_kernel.
constexpr uint32_t kMcWaveRollouts = 32;

template <uint32_t G, bool PLAIN>
__global__ void __launch_bounds__(kBlock) mc_search_kernel(const uint4 *__restrict__ boards, uint32_t n, const McArgs a)
{
    constexpr uint32_t K = G / 4u;
    __shared__ WaveTables s_tables[kBlock / 64];
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const LaneGroup<G> grp;
    const uint32_t j = grp.j, d = grp.d, sub = grp.sub;
    for (uint64_t i = grp.first; i < n; i += grp.stride) {
        const Board in = load_board(boards, static_cast<uint32_t>(i));
        const Board cells = input_cells<PLAIN>(in);
        Board after = cells;
        uint32_t g;
        const bool legal = move_sel(after, tb.move_sel(d), g);
        const uint32_t index = a.index_offset + static_cast<uint32_t>(i);
        uint64_t total = 0;
        uint32_t steps = 0, r = sub; // a lane plays at most R * L < 2^32 moves
        bool live = legal && r < a.rollouts;
        McPlayout p = mc_begin(after);
        if (live)
            total = g;
        while (g2048_any(live)) {
            if (live && mc_trip(p, index, d, r, a.seed_lo, a.seed_hi, a.max_steps, tb, total, steps)) {
                r += K;
                live = r < a.rollouts;
                if (live) {
                    p = mc_begin(after);
                    total += g;
                }
            }
        }
        uint64_t moved = steps;
#pragma unroll
        for (uint32_t o = K / 2u; o > 0u; o >>= 1) {
            total += __shfl_xor(total, o);
            moved += __shfl_xor(moved, o);
        }
        const int64_t value = legal ? static_cast<int64_t>(total) : -1;
        const uint64_t key = group_best_key(root_key<uint64_t>(value, d), K);
        if (sub == 0u && a.value)
            a.value[i * 4u + d] = value;
        if (sub == 0u && a.steps)
            a.steps[i * 4u + d] = legal ? static_cast<int64_t>(moved) : -1;
        if (j == 0u && a.action)
            a.action[i] = static_cast<uint8_t>(root_key_action(key));
    }
}

// ---------------------------------------------------------------------------- n-tuple network
// g2048_ntuple_evaluate: the evaluate definition of g2048_device.h ("n-tuple network value function") for every board.
// A board is a group of four lanes, one per root direction d: lane d moves the board, looks up V of its afterstate --
// 8T gathers whose offsets are all computed before the first load is issued (ntuple_value), so they are in flight
// together -- and the four keys meet in two shuffles.  The lane of the chosen direction writes best, after and
// after_value (lane 0 when no move is legal: every lane then holds the input board).  The cell lists are kernel
// arguments: wave-uniform, so reading a cell of the packed board is a shift by a scalar.  T is a template argument (1..8):
// the look-ups are straight-line code with no per-lane array left at run time.  Lanes stride over the boards when 4n
// exceeds the grid cap (kSearchMaxLanes).  Nothing is written back: no record, clock, episode slot or randomness.
template <uint32_t T, bool PLAIN, class Shape>
__global__ void __launch_bounds__(kBlock) ntuple_eval_kernel(const uint4 *__restrict__ boards, uint32_t n, const Shape sh,
                                                             uint32_t frac_bits, const int32_t *__restrict__ weights,
                                                             const NtupleOut o)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const LaneGroup<4> grp;
    const uint32_t d = grp.d;
    for (uint64_t i = grp.first; i < n; i += grp.stride) {
        const Board in = load_board(boards, static_cast<uint32_t>(i));
        const Board cells = input_cells<PLAIN>(in);
        const NtupleMove m = ntuple_move<T>(cells, d, sh, frac_bits, weights, tb);
        const uint64_t key = group_best_key(ntuple_key(m.q, m.legal, d), 1u);
        const uint32_t action = root_key_action(key);
        const bool any = ntuple_key_legal(key);
        if (o.value)
            o.value[i * 4u + d] = m.q;
        if (d == 0u && o.action)
            o.action[i] = static_cast<uint8_t>(action);
        if (d == (any ? action : 0u)) {
            if (o.best)
                o.best[i] = any ? m.q : 0;
            if (o.after)
                store_board(o.after, static_cast<uint32_t>(i), m.after);
            if (o.after_value)
                o.after_value[i] = any ? m.v : 0;
        }
    }
}

// g2048_ntuple_search: the depth-D search of g2048_device.h ("n-tuple expectimax") for every board.  A board is a
// LaneGroup<G>, K = G / 4 lanes per root direction d; lane `sub` of direction d takes the chance items sub, sub + K, ...
// of that direction's afterstate (ntuple_chance_partial), the K int64 partial sums meet in an xor-shuffle tree, the floor
// division happens once per direction and the four keys meet in group_best_key.  The kernel is gather-latency bound: a
// leaf is four moves of 8T independent loads each, and the only thing that hides their latency is other waves.
// G per depth (kNtupleSearchGroup): 16 at depth 1, where a direction has at most 30 items and K = 4 lanes leave each lane a
// few leaves in a row, and 64 at depth 2, as in expectimax_kernel, where an item is a whole depth-1 tree.  These are the
// starting values: G = 4, 16, 64 at depth 1 and 16, 32, 64 at depth 2 have NOT been timed against each other yet
// (tools/ntuple_search_probe.py --lib times a build with other values; profiles/r12_ntuple_search_probe.txt says what
// was and was not measured).  The weights are read with plain loads and nothing but the outputs is
// written: no record, clock, episode slot or randomness is touched.  Lanes stride over the boards when n * G exceeds the
// grid cap (kSearchMaxLanes); PLAIN as in expectimax_kernel.
template <int D> constexpr uint32_t kNtupleSearchGroup = D == 1 ? 16u : 64u;

template <int D, uint32_t T, bool PLAIN, class Shape, bool MASKED = false>
__global__ void __launch_bounds__(kBlock) ntuple_search_kernel(const uint4 *__restrict__ boards, uint32_t n, const Shape sh,
                                                               uint32_t frac_bits, const int32_t *__restrict__ weights,
                                                               const NtupleSearchOut o)
{
    constexpr uint32_t G = kNtupleSearchGroup<D>, K = G / 4u;
    __shared__ WaveTables s_tables[kBlock / 64];
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const LaneGroup<G> grp;
    const uint32_t j = grp.j, d = grp.d, sub = grp.sub;
    for (uint64_t i = grp.first; i < n; i += grp.stride) {
        const Board in = load_board(boards, static_cast<uint32_t>(i));
        const Board cells = input_cells<PLAIN>(in);
        Board after = cells;
        uint32_t gain;
        bool legal = move_sel(after, tb.move_sel(d), gain);
        // MASKED (g2048_ntuple_search_active): a board the caller masked out has no legal direction -- nothing below is
        // searched and its outputs are those of a dead board.  The G lanes of a group read the same word: wave-uniform at
        // G = 64.  A template parameter, not a test of o.active: the nullable pointer alone moved the register allocation of
        // the unmasked kernels (profiles/r20_ntuple_search_resource_usage.txt).
        if constexpr (MASKED)
            legal = legal && o.active[i] != 0u;
        long long part = 0;
        if (legal)
            part = ntuple_chance_partial<D, T>(after, sub, K, sh, frac_bits, weights, tb);
#pragma unroll
        for (uint32_t x = K / 2u; x > 0u; x >>= 1)
            part += __shfl_xor(part, x);
        // (an illegal direction divides its 0 by 1: its afterstate may have no empty cell)
        const int64_t chance = floor_div(part, legal ? 10 * static_cast<int64_t>(count_empty(after)) : 1);
        const int64_t value = legal ? static_cast<int64_t>(static_cast<uint64_t>(gain) << frac_bits) + chance : kNtupleIllegal;
        const uint64_t key = group_best_key(ntuple_key(value, legal, d), K);
        if (sub == 0u && o.value)
            o.value[i * 4u + d] = value;
        if (j == 0u && o.action)
            o.action[i] = static_cast<uint8_t>(root_key_action(key));
    }
}

// g2048_ntuple_deep_search: the depth-D search, D = 2..3, with ONE WORKGROUP (kBlock lanes, four wavefronts) per board -- the
// steps of g2048_device.h ("n-tuple deep search") with a barrier after each.  In ntuple_search_kernel a lane walks its chance
// items one after the other; at depth 3 an item would be a whole depth-2 tree on one lane.  Here the level-1 items and their
// afterstates (at most 480) are laid out in LDS once, and all 256 lanes share the list of their chance items, each a
// depth-1 tree at depth 3 and one evaluate at depth 2: the straight-line code of ntuple_search_state<D - 2>.  A lane adds
// its weight * S to the entry's int64 in LDS with one 64-bit LDS atomic per unit (hundreds of gathers stand behind each add);
// integer adds commute, so the bits
// do not depend on who took which unit.  LDS: sizeof(NtupleDeepLds) + the wave tables, about 18 KB, static.  Workgroups
// stride over the boards when n * kBlock exceeds the grid cap (kSearchMaxLanes): at most 65 536 workgroups.  Nothing but the
// outputs is written.  MASKED: a board at 0 in o.active has no legal root direction (ntuple_deep_root), so every step finds
// nothing to do and finish writes the outputs of a dead board -- the path the host check runs; no barrier is skipped.
// Measured on the MI355X (profiles/r21_ntuple_deep_probe.txt): depth 3 of 1 024 late-game boards (1..4 empty cells), 4x6 network:
// 14.6 ms per launch against 53.0 ms for ntuple_search_kernel<3> (the same template at one wavefront per board), 2.9 to 4.3
// times faster over both networks and 1 024 / 4 096 boards, which is why this kernel and not that instantiation is shipped; at
// depth 2 it takes 0.32 to 0.61 of the existing kernel's time at 1 024 boards (recorded; g2048_ntuple_search is unchanged).
// Not measured: other block sizes, a finer split of a unit, T other than 4 and 8, occupancy-limited shapes against each other.
template <int D, uint32_t T, bool PLAIN, class Shape, bool MASKED = false>
__global__ void __launch_bounds__(kBlock) ntuple_deep_search_kernel(const uint4 *__restrict__ boards, uint32_t n, const Shape sh,
                                                                    uint32_t frac_bits, const int32_t *__restrict__ weights,
                                                                    const NtupleSearchOut o)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    __shared__ NtupleDeepLds s_deep;
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const uint32_t lane = threadIdx.x;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) { // (64 bits: n may be within one grid of 2^32)
        // MASKED: the board's root directions count as illegal, so it has no items, no entries and no units: every step below
        // falls through and finish writes the outputs of a dead board.  The word is the same for the whole workgroup.
        bool active = true;
        if constexpr (MASKED)
            active = o.active[i] != 0u;
        const Board cells = input_cells<PLAIN>(load_board(boards, static_cast<uint32_t>(i)));
        ntuple_deep_root(s_deep, cells, active, lane, tb);
        __syncthreads();
        ntuple_deep_expand(s_deep, lane, kBlock, tb);
        __syncthreads();
        ntuple_deep_scan(s_deep, lane, kBlock);
        __syncthreads();
        ntuple_deep_leaves<D, T>(s_deep, lane, kBlock, sh, frac_bits, weights, tb, [&](uint32_t e, int64_t x) {
            atomicAdd(reinterpret_cast<unsigned long long *>(&s_deep.acc[e]), static_cast<unsigned long long>(x));
        });
        __syncthreads();
        ntuple_deep_fold(s_deep, lane, kBlock, frac_bits, [&](uint32_t d1, int64_t x) {
            atomicAdd(reinterpret_cast<unsigned long long *>(&s_deep.root_sum[d1]), static_cast<unsigned long long>(x));
        });
        __syncthreads();
        if (lane == 0u) {
            int64_t value[4];
            const uint32_t action = ntuple_deep_finish(s_deep, frac_bits, value);
            if (o.value) {
#pragma unroll
                for (uint32_t d = 0; d < 4u; ++d)
                    o.value[i * 4u + d] = value[d];
            }
            if (o.action)
                o.action[i] = static_cast<uint8_t>(action);
        }
        __syncthreads(); // the next board's root step overwrites what lane 0 reads above
    }
}

// g2048_ntuple_adaptive_search: ntuple_deep_search_kernel with a depth per board, D = schedule[E0(board)] in 0..4 -- the steps of
// g2048_device.h ("n-tuple adaptive search") with a barrier after each.  D is a run-time value, the same for the whole
// workgroup: every branch on it is wave-uniform and every barrier is reached by all 256 lanes or by none.  One kernel per
// (T, shape, plain / engine / masked) holds the leaves of all depths, S_0, S_1 and S_2 on a lane, so its registers are those of
// its deepest leaf, ntuple_search_state<2>, whatever schedule a launch runs: 24 to 26 VGPRs above ntuple_deep_search_kernel<3>
// and, at T = 1..6, one or two waves per SIMD fewer (profiles/r23_ntuple_adaptive_resource_usage.txt).  A second form of the
// kernel without the depth-4 unit, for schedules that hold no 4, was built and timed on the MI355X: with the registers and the
// occupancy of the deep kernel it was no faster at T = 8 and SLOWER at T = 4 than this one (by 3 % on late-game and 12 % on
// mid-game boards, profiles/r23_ntuple_adaptive_probe.txt), so it is not kept.
// AdaptiveTables: LdsTables under a type of this kernel's own, so that the device templates it instantiates
// (ntuple_chance_partial<2, ..> and the lambdas in it) are not the instantiations of ntuple_search_kernel -- shared, the
// compiler inlined them in another order there and those 72 kernels came out with other register counts than the parent's.
// LDS, the grid cap, the stride loop and MASKED as in ntuple_deep_search_kernel; a masked-out board skips nothing but work.
struct AdaptiveTables : LdsTables {};

template <uint32_t T, bool PLAIN, class Shape, bool MASKED = false>
__global__ void __launch_bounds__(kBlock) ntuple_adaptive_search_kernel(const uint4 *__restrict__ boards, uint32_t n, const Shape sh,
                                                                        uint32_t frac_bits, const int32_t *__restrict__ weights,
                                                                        const NtupleAdaptiveSchedule schedule, const NtupleAdaptiveOut o)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    __shared__ NtupleDeepLds s_deep;
    const AdaptiveTables tb{stage_tables(s_tables, load_tables_piece())};
    const uint32_t lane = threadIdx.x;
    const auto add_root = [&](uint32_t d1, int64_t x) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&s_deep.root_sum[d1]), static_cast<unsigned long long>(x));
    };
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) { // (64 bits: n may be within one grid of 2^32)
        bool active = true;
        if constexpr (MASKED)
            active = o.active[i] != 0u;
        const Board cells = input_cells<PLAIN>(load_board(boards, static_cast<uint32_t>(i)));
        const uint32_t depth = ntuple_adaptive_depth(schedule, cells);
        ntuple_adaptive_root<T>(s_deep, cells, active, depth, lane, sh, weights, tb);
        __syncthreads();
        if (depth == 1u) {
            ntuple_adaptive_leaves1<T>(s_deep, lane, kBlock, sh, frac_bits, weights, tb, add_root);
            __syncthreads();
        } else if (depth >= 2u) {
            ntuple_deep_expand(s_deep, lane, kBlock, tb);
            __syncthreads();
            ntuple_deep_scan(s_deep, lane, kBlock);
            __syncthreads();
            ntuple_adaptive_leaves<T>(s_deep, depth, lane, kBlock, sh, frac_bits, weights, tb, [&](uint32_t e, int64_t x) {
                atomicAdd(reinterpret_cast<unsigned long long *>(&s_deep.acc[e]), static_cast<unsigned long long>(x));
            });
            __syncthreads();
            ntuple_deep_fold(s_deep, lane, kBlock, frac_bits, add_root);
            __syncthreads();
        }
        if (lane == 0u) {
            int64_t value[4];
            const uint32_t action = ntuple_adaptive_finish(s_deep, depth, frac_bits, value);
            if (o.value) {
#pragma unroll
                for (uint32_t d = 0; d < 4u; ++d)
                    o.value[i * 4u + d] = value[d];
            }
            if (o.action)
                o.action[i] = static_cast<uint8_t>(action);
            if (o.depth)
                o.depth[i] = static_cast<uint8_t>(active ? depth : kNtupleAdaptiveSkipped);
        }
        __syncthreads(); // the next board's root step overwrites what lane 0 reads above
    }
}

// g2048_ntuple_reduced_search: ntuple_adaptive_search_kernel with the children of a 4 spawn searched `reduce4` plies shallower
// -- the steps of g2048_device.h ("n-tuple reduced search") with a barrier after each.  The depth is a run-time value of the
// workgroup and reduce4 one of the launch: every branch on them around a barrier is wave-uniform.  Depths 0 and 1 run the
// adaptive steps.  At depth 2..4 the units of a board differ by up to two plies; a lane runs ntuple_reduced_state, ONE loop
// nest with run-time depths that holds three bodies of the look-up where the adaptive kernel's S_0, S_1 and S_2 hold six, so
// lanes of unequal depth share instructions.  The deepest path is still three nested move loops on a lane, and the registers
// and waves per SIMD are the adaptive kernel's to within 1 VGPR (profiles/r27_ntuple_reduced_resource_usage.txt).
// Measured on the MI355X (profiles/r27_ntuple_reduced_probe.txt): depth 4 of 1 024 late-game boards, 4x6 network, 371 ms per
// launch against the adaptive kernel's 918 ms with 0.15 of its evaluations; depth 3 takes 0.80 (reduce4 = 1) or 0.47 (2) of its
// time with 0.28.  The units are NOT ordered by depth: every chance entry starts at an even unit, so an even lane always draws
// a 2 child and an odd lane a 4 child, and half of every wavefront waits for the deeper half -- which is what the rows point to;
// ordering them in the scan was not built and not timed.  ReducedTables: as AdaptiveTables, so that this kernel shares no
// template instantiation with the existing ones.  LDS, the grid cap, the stride loop and MASKED as in ntuple_deep_search_kernel.
struct ReducedTables : LdsTables {};

template <uint32_t T, bool PLAIN, class Shape, bool MASKED = false>
__global__ void __launch_bounds__(kBlock) ntuple_reduced_search_kernel(const uint4 *__restrict__ boards, uint32_t n, const Shape sh,
                                                                       uint32_t frac_bits, const int32_t *__restrict__ weights,
                                                                       const NtupleAdaptiveSchedule schedule, uint32_t reduce4,
                                                                       const NtupleAdaptiveOut o)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    __shared__ NtupleDeepLds s_deep;
    const ReducedTables tb{stage_tables(s_tables, load_tables_piece())};
    const uint32_t lane = threadIdx.x;
    const auto add_root = [&](uint32_t d1, int64_t x) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&s_deep.root_sum[d1]), static_cast<unsigned long long>(x));
    };
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) { // (64 bits: n may be within one grid of 2^32)
        bool active = true;
        if constexpr (MASKED)
            active = o.active[i] != 0u;
        const Board cells = input_cells<PLAIN>(load_board(boards, static_cast<uint32_t>(i)));
        const uint32_t depth = ntuple_adaptive_depth(schedule, cells);
        ntuple_adaptive_root<T>(s_deep, cells, active, depth, lane, sh, weights, tb);
        __syncthreads();
        if (depth == 1u) {
            ntuple_adaptive_leaves1<T>(s_deep, lane, kBlock, sh, frac_bits, weights, tb, add_root);
            __syncthreads();
        } else if (depth >= 2u) {
            ntuple_reduced_expand(s_deep, depth, reduce4, lane, kBlock, tb);
            __syncthreads();
            ntuple_deep_scan(s_deep, lane, kBlock);
            __syncthreads();
            ntuple_reduced_leaves<T>(s_deep, depth, reduce4, lane, kBlock, sh, frac_bits, weights, tb, [&](uint32_t e, int64_t x) {
                atomicAdd(reinterpret_cast<unsigned long long *>(&s_deep.acc[e]), static_cast<unsigned long long>(x));
            });
            __syncthreads();
            ntuple_reduced_fold(s_deep, lane, kBlock, frac_bits, add_root);
            __syncthreads();
        }
        if (lane == 0u) {
            int64_t value[4];
            const uint32_t action = ntuple_adaptive_finish(s_deep, depth, frac_bits, value);
            if (o.value) {
#pragma unroll
                for (uint32_t d = 0; d < 4u; ++d)
                    o.value[i * 4u + d] = value[d];
            }
            if (o.action)
                o.action[i] = static_cast<uint8_t>(action);
            if (o.depth)
                o.depth[i] = static_cast<uint8_t>(active ? depth : kNtupleAdaptiveSkipped);
        }
        __syncthreads(); // the next board's root step overwrites what lane 0 reads above
    }
}

// g2048_ntuple_values_plain: V of every board, one board per lane, the same gathers.
template <uint32_t T, class Shape>
__global__ void __launch_bounds__(kBlock) ntuple_values_kernel(const uint4 *__restrict__ boards, uint32_t n, const Shape sh,
                                                               const int32_t *__restrict__ weights, int64_t *__restrict__ v)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    v[i] = ntuple_value<T>(ntuple_pack(load_board(boards, i)), sh, weights);
}

// g2048_ntuple_stage_plain: stage(b) of every board, one board per lane; no table is read.
__global__ void __launch_bounds__(kBlock) ntuple_stage_kernel(const uint4 *__restrict__ boards, uint32_t n, const NtupleStagedShape sh,
                                                              uint8_t *__restrict__ stage)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    stage[i] = static_cast<uint8_t>(ntuple_stage(ntuple_stage_mask(ntuple_pack(load_board(boards, i))), sh));
}

// g2048_ntuple_play: k_steps of the greedy player (ntuple_play_step of g2048_device.h) with auto-reset in ONE launch; the
// record never leaves registers, as in rollout_random_kernel, whose bookkeeping this is: record_episode_ends, then
// reset_record, per step; the lane's gains folded every kGainFold steps; one record store and one flush_episode_counts at the
// end.  One board per lane, 64 boards per wavefront -- the episode slot is private to the wavefront of boards 64w .. 64w + 63
// and written without atomics, so the four-lanes-per-board layout of ntuple_eval_kernel (four wavefronts per slot) is not an
// option: a lane does its four directions itself (ntuple_root), up to 32T gathers per move, all offsets of a direction
// computed before its first load (ntuple_value).  The weights are read with plain loads; nothing in the launch writes them.
// The side outputs (NtuplePlayOut, any of them NULL): a board whose games_left entry is 0 when a step begins sits that step
// out -- record untouched, no gain, no episode end, nothing counted -- and an entry drops by one when the board's episode
// ends, after the reset, so a board that runs out rests on its fresh board; hist[highest exponent of the terminal board] += 1
// per episode end, one atomic per ending lane (rare); moves += the (board, step) pairs played, summed over the wave first:
// one atomic per wave per launch.  Integer adds: the same bits for any launch geometry.  A wavefront none of whose boards
// has a game left stops stepping (nothing it could still do is visible: t is the launch's, not the lane's).
template <uint32_t T, class Shape>
__global__ void __launch_bounds__(kBlock) ntuple_play_kernel(const StepArgs p, const Shape sh, uint32_t frac_bits,
                                                             const int32_t *__restrict__ weights, const NtuplePlayOut io)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const Lane ln = lane_of<kBlock, false>(p.n);
    Board rec = load_board(p.st.boards, ln.i);
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    uint32_t left = io.games_left ? io.games_left[ln.i] : 1u; // (no limit: never decremented)
    uint64_t t = (static_cast<uint64_t>(p.t_hi) << 32) | p.t_lo; // transaction of the first step
    uint32_t episodes = 0, illegal_ends = 0, played = 0, gained32 = 0;
    unsigned long long gained = 0; // as in rollout_random_kernel: 32-bit adds, folded into 64 bits every kGainFold steps
    for (uint32_t j = 0; j < p.k_steps; ++j, ++t) {
        const bool go = left != 0u;
        if (__builtin_amdgcn_ballot_w64(go) == 0ull)
            break;
        StepOut o{}; // a board that sits the step out: gain 0, not terminated
        Words w{};
        if (go)
            o = ntuple_play_step<T>(rec, t, p.board_offset + ln.i, p.seed_lo, p.seed_hi, sh, frac_bits, weights, p.max_exp, tb, w);
        played += go ? 1u : 0u;
        gained32 += o.gain;
        const bool fin = o.terminated && ln.valid;
        record_episode_ends(p, ln.i, fin, !o.legal, rec, episodes, illegal_ends);
        if (o.terminated) {
            if (fin && io.hist)
                atomicAdd(io.hist + highest(record_cells(rec)), 1ull);
            reset_record(rec, o, w, tb);
            if (io.games_left)
                left -= 1u;
        }
        if ((j + 1u) % kGainFold == 0u) {
            gained += gained32;
            gained32 = 0;
        }
    }
    gained += gained32;
    if (ln.valid) {
        store_board(p.st.boards, ln.i, rec);
        if (io.games_left)
            io.games_left[ln.i] = left;
    }
    // a board that was stepped has been reset at every episode end; one that sat the whole launch out keeps its mark
    const unsigned long long pending = ((static_cast<unsigned long long>(counters.pend_hi) << 32) | counters.pend_lo) &
                                       ~__builtin_amdgcn_ballot_w64(played != 0u);
    flush_episode_counts(counters, episodes, illegal_ends, wave_sum64_lane63(ln.valid ? gained : 0ull), pending);
    if (io.moves) { // (wave-uniform)
        const unsigned long long total = wave_sum64_lane63(ln.valid ? played : 0u);
        if ((threadIdx.x & 63u) == 63u && total != 0ull)
            atomicAdd(io.moves, total);
    }
}

// g2048_ntuple_play_downgraded: ntuple_play_kernel with the action taken on the translated cells of the record
// (ntuple_play_downgraded_step of g2048_device.h) -- the same lane layout, the same bookkeeping, the same side outputs, all of
// them describing the real game.  The body is ntuple_play_kernel's, copied: a flag in that kernel, or its body shared as a
// __device__ function, would move the register allocation of its 24 instantiations (what happened with play_step_kernel,
// below), so that kernel stays as it was and this one has 24 of its own (profiles/r30_downgrade_resource_usage.txt).
template <uint32_t T, class Shape>
__global__ void __launch_bounds__(kBlock) ntuple_play_downgraded_kernel(const StepArgs p, const Shape sh, uint32_t frac_bits,
                                                                        const int32_t *__restrict__ weights, const DowngradeRule rule,
                                                                        const NtuplePlayOut io)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const Lane ln = lane_of<kBlock, false>(p.n);
    Board rec = load_board(p.st.boards, ln.i);
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    uint32_t left = io.games_left ? io.games_left[ln.i] : 1u; // (no limit: never decremented)
    uint64_t t = (static_cast<uint64_t>(p.t_hi) << 32) | p.t_lo; // transaction of the first step
    uint32_t episodes = 0, illegal_ends = 0, played = 0, gained32 = 0;
    unsigned long long gained = 0; // as in ntuple_play_kernel: 32-bit adds, folded into 64 bits every kGainFold steps
    for (uint32_t j = 0; j < p.k_steps; ++j, ++t) {
        const bool go = left != 0u;
        if (__builtin_amdgcn_ballot_w64(go) == 0ull)
            break;
        StepOut o{}; // a board that sits the step out: gain 0, not terminated
        Words w{};
        if (go)
            o = ntuple_play_downgraded_step<T>(rec, t, p.board_offset + ln.i, p.seed_lo, p.seed_hi, sh, frac_bits, weights, p.max_exp,
                                               rule, tb, w);
        played += go ? 1u : 0u;
        gained32 += o.gain;
        const bool fin = o.terminated && ln.valid;
        record_episode_ends(p, ln.i, fin, !o.legal, rec, episodes, illegal_ends);
        if (o.terminated) {
            if (fin && io.hist)
                atomicAdd(io.hist + highest(record_cells(rec)), 1ull);
            reset_record(rec, o, w, tb);
            if (io.games_left)
                left -= 1u;
        }
        if ((j + 1u) % kGainFold == 0u) {
            gained += gained32;
            gained32 = 0;
        }
    }
    gained += gained32;
    if (ln.valid) {
        store_board(p.st.boards, ln.i, rec);
        if (io.games_left)
            io.games_left[ln.i] = left;
    }
    // a board that was stepped has been reset at every episode end; one that sat the whole launch out keeps its mark
    const unsigned long long pending = ((static_cast<unsigned long long>(counters.pend_hi) << 32) | counters.pend_lo) &
                                       ~__builtin_amdgcn_ballot_w64(played != 0u);
    flush_episode_counts(counters, episodes, illegal_ends, wave_sum64_lane63(ln.valid ? gained : 0ull), pending);
    if (io.moves) { // (wave-uniform)
        const unsigned long long total = wave_sum64_lane63(ln.valid ? played : 0u);
        if ((threadIdx.x & 63u) == 63u && total != 0ull)
            atomicAdd(io.moves, total);
    }
}

// g2048_downgrade_plain / g2048_downgrade_boards: downgrade_cells of every board, one board per lane, 16 B in and 16 (+ 1) B
// out; no LDS, no table.  `boards` are plain boards or engine records (the rule masks every byte to its cell), and `out` may be
// `boards`: a lane reads its board before it writes it, and no lane reads another's (so neither pointer is __restrict__).
// active (NULL: every board): a board at 0 gets the all-empty board and kDowngradeSkipped.
__global__ void __launch_bounds__(kBlock) downgrade_kernel(const uint4 *boards, uint32_t n, const DowngradeRule rule,
                                                           const uint32_t *__restrict__ active, uint4 *out, uint8_t *__restrict__ missing)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    Downgraded d = downgrade_cells(load_board(boards, i), rule);
    if (active && active[i] == 0u) // (active: wave-uniform)
        d = Downgraded{Board{{0u, 0u, 0u, 0u}}, kDowngradeSkipped};
    store_board(out, i, d.cells);
    if (missing)
        missing[i] = static_cast<uint8_t>(d.k);
}

// g2048_play_step: ONE step of every board under that contract with the action read from a buffer (ACT as in step_kernel: 0 =
// the synthetic policy of the transaction, 1 / 2 / 3 = uint8 / int32 / int64) -- g2048_ntuple_play with k_steps == 1 for any
// player.  The same lane layout for the same reason: one board per lane, the wavefront owns its episode slot.  The body is
// ntuple_play_kernel's per-step body, copied, with the action loaded instead of computed and no loop around it: sharing it
// as one __device__ function moved the register allocation of 19 of ntuple_play_kernel's 24 instantiations
// (profiles/r20_play_step_resource_usage.txt), so that kernel stays as it was.  A board that rests is not checked for an
// action outside 0..3 either (strict actions): its entry is loaded -- the buffer holds n -- and dropped.  No step output.
template <int ACT>
__global__ void __launch_bounds__(kBlock) play_step_kernel(const StepArgs p, const NtuplePlayOut io)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const Lane ln = lane_of<kBlock, false>(p.n);
    Board rec = load_board(p.st.boards, ln.i);
    const auto raw = load_action_at<ACT>(p.actions, ln.i);
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    uint32_t left = io.games_left ? io.games_left[ln.i] : 1u; // (no limit: never decremented)
    uint32_t episodes = 0, illegal_ends = 0;
    const bool go = left != 0u;
    StepOut o{}; // a board that sits the step out: gain 0, not terminated
    Words w{};
    BadAction bad; // (stays unset on a board that rests)
    if (go) {
        w = philox4x32_10(p.t_lo, p.t_hi, p.board_offset + ln.i, 0u, p.seed_lo, p.seed_hi);
        uint32_t action;
        if constexpr (ACT == 0)
            action = w.w[3] >> 30;
        else
            action = bad.note_only(raw);
        o = play_record(rec, action, w, p.max_exp, tb);
    }
    const bool fin = o.terminated && ln.valid;
    record_episode_ends(p, ln.i, fin, !o.legal, rec, episodes, illegal_ends);
    if (o.terminated) {
        if (fin && io.hist)
            atomicAdd(io.hist + highest(record_cells(rec)), 1ull);
        reset_record(rec, o, w, tb);
        if (io.games_left)
            left -= 1u;
    }
    if (ln.valid) {
        store_board(p.st.boards, ln.i, rec);
        if (io.games_left)
            io.games_left[ln.i] = left;
    }
    // a board that was stepped has been reset if its episode ended; one that sat the step out keeps its mark
    const unsigned long long played = __builtin_amdgcn_ballot_w64(go);
    const unsigned long long pending = ((static_cast<unsigned long long>(counters.pend_hi) << 32) | counters.pend_lo) & ~played;
    flush_episode_counts(counters, episodes, illegal_ends, wave_sum_lane63(ln.valid ? o.gain : 0u), pending);
    if (io.moves) { // (wave-uniform)
        const unsigned long long total = static_cast<unsigned long long>(__popcll(played & __builtin_amdgcn_ballot_w64(ln.valid)));
        if ((threadIdx.x & 63u) == 63u && total != 0ull)
            atomicAdd(io.moves, total);
    }
    if constexpr (ACT != 0) {
        if (p.action_err) // (wave-uniform)
            report_bad_action(p.action_err, bad.bad && ln.valid, bad.raw, p.board_offset + ln.i);
    }
}

// g2048_ntuple_td_step: the front half of every n-tuple learner in ONE launch (ntuple_td_step of g2048_device.h) -- evaluate,
// play the greedy move with auto-reset, evaluate the board that is then live, form the error.  ntuple_play_kernel's lane
// layout for its reason (one board per lane, the wavefront owns its episode slot) and its per-step bookkeeping at
// k_steps == 1 without a budget: record_episode_ends, then reset_record, one record store, one flush_episode_counts; every
// board is stepped and reset if its episode ended, so no pending mark survives the launch.  A kernel of its own, sharing only
// what ntuple_play_kernel already calls: that kernel and play_step_kernel keep their register allocation
// (profiles/r25_ntuple_td_resource_usage.txt).  A lane does both roots itself, up to 64T gathers; the weights are read with
// plain loads, nothing in the launch writes them.  The outputs (NtupleTdIo, any of them NULL) are the lane's own entries.
template <uint32_t T, class Shape>
__global__ void __launch_bounds__(kBlock) ntuple_td_step_kernel(const StepArgs p, const Shape sh, uint32_t frac_bits,
                                                                const int32_t *__restrict__ weights, const NtupleTdIo io)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    const Lane ln = lane_of<kBlock, false>(p.n);
    Board rec = load_board(p.st.boards, ln.i);
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    const uint64_t t = (static_cast<uint64_t>(p.t_hi) << 32) | p.t_lo;
    uint32_t episodes = 0, illegal_ends = 0;
    const NtupleTdOut o = ntuple_td_step<T>(rec, t, p.board_offset + ln.i, p.seed_lo, p.seed_hi, sh, frac_bits, weights, p.max_exp, tb,
                                            [&](const StepOut &st, const Board &terminal) { // (whole wavefronts: a ballot inside)
                                                record_episode_ends(p, ln.i, st.terminated && ln.valid, !st.legal, terminal, episodes,
                                                                    illegal_ends);
                                            });
    if (ln.valid) {
        store_board(p.st.boards, ln.i, rec);
        if (io.action)
            io.action[ln.i] = static_cast<uint8_t>(o.action);
        if (io.after)
            store_board(io.after, ln.i, o.after);
        if (io.after_value)
            io.after_value[ln.i] = o.after_value;
        if (io.best_next)
            io.best_next[ln.i] = o.best_next;
        if (io.terminated)
            io.terminated[ln.i] = static_cast<uint8_t>(o.step.terminated ? 1 : 0);
        if (io.delta)
            io.delta[ln.i] = o.delta;
    }
    flush_episode_counts(counters, episodes, illegal_ends, wave_sum_lane63(ln.valid ? o.step.gain : 0u), 0ull);
}

// g2048_ntuple_play_log: ntuple_play_kernel without a budget -- log.depth moves of the greedy player in ONE launch, the record
// in registers, the same bookkeeping (record_episode_ends, then reset_record, per move; the gains folded every kGainFold moves;
// one record store and one flush_episode_counts at the end; every board is stepped, so no pending mark survives) -- that also
// leaves every move in the log (ntuple_play_log_step of g2048_device.h: ntuple_root_kept keeps the afterstate and both values
// by selects, no array indexed by the action).  The per-move body is ntuple_play_kernel's, copied: shared as a __device__
// function it would move that kernel's register allocation (the comment above play_step_kernel).  One board per lane for
// ntuple_play_kernel's reason, so the stores of a move are slot-major and whole: a wavefront writes 1 KiB contiguous of
// `after`, 512 B of `gain` and 64 B of `flag`.  First the carry: slot 0 takes the three entries slot M held, each lane its own
// board's (M >= 1: the two slots differ, and no lane reads what another writes).  Slot bases are formed in 64 bits:
// (M + 1) * n * 16 bytes exceeds 2^32.  The weights are read with plain loads; nothing in the launch writes them.
// RESTART (g2048_ntuple_play_log_restart): restart_board of g2048_device.h behind every move, on the record in registers, with
// pos, start and restarts of the board held in registers over the M moves and stored once -- the bits of M rounds of
// evaluate -> step -> g2048_restart_step.  A lane past the end neither reads nor writes the snapshots.  A compile-time option:
// without it the body is what ntuple_play_log_kernel was, and `rs` is not looked at.
struct NoRestart {};
template <uint32_t T, bool RESTART, class Shape, class Rs>
__device__ __forceinline__ void ntuple_play_log_body(WaveTables *s_tables, const StepArgs &p, const Shape &sh, uint32_t frac_bits,
                                                     const int32_t *__restrict__ weights, const NtupleLog &log, const Rs &rs)
{
    const Lane ln = lane_of<kBlock, false>(p.n);
    Board rec = load_board(p.st.boards, ln.i);
    const LdsTables tb = stage_tables(s_tables, load_tables_piece());
    const EpisodeCounters counters = load_episode_counters(p, ln.i_raw);
    if (ln.valid) { // the carry
        const uint64_t last = static_cast<uint64_t>(log.depth) * p.n;
        store_board(log.after, ln.i, load_board(log.after + last, ln.i));
        log.gain[ln.i] = log.gain[last + ln.i];
        log.flag[ln.i] = log.flag[last + ln.i];
    }
    RestartBoard rb{};
    if constexpr (RESTART)
        rb = RestartBoard{rs.pos[ln.i], rs.start[ln.i], rs.restarts[ln.i]};
    uint64_t t = (static_cast<uint64_t>(p.t_hi) << 32) | p.t_lo; // transaction of the first move
    uint32_t episodes = 0, illegal_ends = 0, gained32 = 0;
    unsigned long long gained = 0; // as in ntuple_play_kernel: 32-bit adds, folded into 64 bits every kGainFold moves
    for (uint32_t m = 1; m <= log.depth; ++m, ++t) {
        Words w;
        NtupleLogEntry e;
        const StepOut o = ntuple_play_log_step<T>(rec, t, p.board_offset + ln.i, p.seed_lo, p.seed_hi, sh, frac_bits, weights, p.max_exp,
                                                  tb, w, e);
        if (ln.valid) {
            const uint64_t slot = static_cast<uint64_t>(m) * p.n;
            store_board(log.after + slot, ln.i, e.after);
            log.gain[slot + ln.i] = e.gain;
            log.flag[slot + ln.i] = static_cast<uint8_t>(e.flag);
        }
        gained32 += o.gain;
        const bool fin = o.terminated && ln.valid;
        record_episode_ends(p, ln.i, fin, !o.legal, rec, episodes, illegal_ends);
        if (o.terminated)
            reset_record(rec, o, w, tb);
        if constexpr (RESTART) {
            if (ln.valid)
                restart_board(RestartRecordHeld{rec}, o.terminated, rs.rule, rs.snap, p.n, ln.i, rb);
        }
        if (m % kGainFold == 0u) {
            gained += gained32;
            gained32 = 0;
        }
    }
    gained += gained32;
    if (ln.valid) {
        store_board(p.st.boards, ln.i, rec);
        if constexpr (RESTART) {
            rs.pos[ln.i] = rb.pos;
            rs.start[ln.i] = rb.start;
            rs.restarts[ln.i] = rb.restarts;
        }
    }
    flush_episode_counts(counters, episodes, illegal_ends, wave_sum64_lane63(ln.valid ? gained : 0ull), 0ull);
}

template <uint32_t T, class Shape>
__global__ void __launch_bounds__(kBlock) ntuple_play_log_kernel(const StepArgs p, const Shape sh, uint32_t frac_bits,
                                                                 const int32_t *__restrict__ weights, const NtupleLog log)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    ntuple_play_log_body<T, false>(s_tables, p, sh, frac_bits, weights, log, NoRestart{});
}

template <uint32_t T, class Shape>
__global__ void __launch_bounds__(kBlock) ntuple_play_log_restart_kernel(const StepArgs p, const Shape sh, uint32_t frac_bits,
                                                                         const int32_t *__restrict__ weights, const NtupleLog log,
                                                                         const Restart rs)
{
    __shared__ WaveTables s_tables[kBlock / 64];
    ntuple_play_log_body<T, true>(s_tables, p, sh, frac_bits, weights, log, rs);
}

// g2048_restart_step: restart_board of g2048_device.h, one board per lane in a grid-stride loop (at most kRestartMaxGroups
// workgroups whatever n is), ONE launch.  A board whose episode goes on reads terminated[i] and pos[i] and writes pos[i]; on
// one step in s it also reads its record and stores it in a slot -- slot-major, so a wavefront stores 1 KiB contiguous.  A
// board whose episode ended reads start[i] and restarts[i] too and, when it restarts, loads one slot and stores its record.
// Every lane touches its own board's state only: nothing a lane reads is written by another.
__global__ void __launch_bounds__(kBlock) restart_step_kernel(uint4 *__restrict__ records, const uint8_t *__restrict__ terminated, uint32_t n,
                                                              const Restart rs)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; g < n; g += stride) {
        const uint32_t i = static_cast<uint32_t>(g);
        const bool ended = terminated[i] != 0;
        RestartBoard b{rs.pos[i], 0u, 0u};
        const uint32_t pos = b.pos;
        if (ended) {
            b.start = rs.start[i];
            b.restarts = rs.restarts[i];
        }
        restart_board(RestartRecordStored{records, i}, ended, rs.rule, rs.snap, n, i, b);
        if (b.pos != pos)
            rs.pos[i] = b.pos;
        if (ended) {
            rs.start[i] = b.start;
            rs.restarts[i] = b.restarts;
        }
    }
}

// g2048_ntuple_log_delta: the backward error of slot m (ntuple_log_delta of g2048_device.h), one board per lane as
// ntuple_values_kernel, whose V this is (ntuple_value on the packed board).  Up to two evaluations per board, 16T gathers; each
// sits behind the flags that ask for it, so a wavefront whose boards all ended, or all have no successor, skips the second,
// and one whose boards are all empty skips both.  The four-lanes-per-board layout of ntuple_eval_kernel is for the four
// directions of one board; here there are two boards and no move to make, and one lane per board keeps the loads of a slot
// contiguous over the wave (1 KiB of `after`, 512 B of `gain`, 64 B of `flag`) and the stores of delta whole.  A lane reads
// flag[m], flag[m + 1], and what they ask for; it writes delta[i] only -- nothing it reads is written in the launch.
// The two evaluations are straight-line code.  As one body in a two-trip loop (#pragma nounroll) the kernel holds 35 to 150
// VGPRs in every shape where this form holds up to 243 (staged, T = 3..5), but it spills up to 634 SGPRs to VGPR lanes and
// was slower in 11 of the 12 rows timed, by 1 to 5 us per launch (profiles/r28_ntuple_log_resource_usage.txt).
template <uint32_t T, class Shape>
__global__ void __launch_bounds__(kBlock) ntuple_log_delta_kernel(const NtupleLog log, uint32_t n, uint32_t m, const Shape sh,
                                                                  const int32_t *__restrict__ weights, int64_t *__restrict__ delta)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t self = static_cast<uint64_t>(m) * n, next = self + n;
    const uint32_t f = log.flag[self + i], f1 = log.flag[next + i];
    int64_t v0 = 0, v1 = 0, gain1 = 0;
    if (ntuple_log_reads_self(f, f1))
        v0 = ntuple_value<T>(ntuple_pack(load_board(log.after + self, i)), sh, weights);
    if (ntuple_log_reads_next(f, f1)) {
        gain1 = log.gain[next + i];
        v1 = ntuple_value<T>(ntuple_pack(load_board(log.after + next, i)), sh, weights);
    }
    delta[i] = ntuple_log_delta(f, f1, gain1, v1, v0);
}

// The nine updates (g2048_ntuple_update_plain, g2048_ntuple_tc_update_plain, g2048_ntuple_trace_update,
// g2048_ntuple_tc_trace_update, g2048_ntuple_delay_update, g2048_ntuple_tc_delay_update; the definitions of g2048_device.h,
// "n-tuple network value function", "Temporal-coherence learning", "n-tuple traces" and "n-tuple delay") are three kernels,
// each over one of the item sources of g2048_device.h ("The work items of an update"): NtupleBoardItems, one board per item,
// NtupleTraceItems or NtupleDelayItems, one (k, i) per item.  A kernel is the header's item
// loop and per-item operation with an atomic add: relaxed, agent scope, its result read by nobody (fire and forget).
// Integer adds commute, so the tables after a launch do not depend on the order the lanes, waves or launches arrive in.
// A lane takes the items lane, lane + grid, ...: the grid is capped at kSearchMaxLanes.  delta is an argument of its own, and
// __restrict__: as a member of the source, phase W over a trace took 24 and 40 more VGPRs at T = 2 and 3 and lost a wave
// (profiles/r16_ntuple_items_resource_usage.txt).
struct AtomicAddWeights { // weights[off] += step, wrapping mod 2^32
    uint32_t *w;
    __device__ void operator()(uint32_t off, int32_t step) const
    {
        __hip_atomic_fetch_add(w + off, static_cast<uint32_t>(step), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct AtomicAddAccum { // err[off] += d, mag[off] += |d|, wrapping mod 2^64
    unsigned long long *e, *a;
    __device__ void operator()(uint32_t off, int64_t d, uint64_t m) const
    {
        __hip_atomic_fetch_add(e + off, static_cast<unsigned long long>(d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(a + off, static_cast<unsigned long long>(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// f(item) for every item of this lane
template <class Items, class F> __device__ __forceinline__ void lane_items(const Items &items, F f)
{
    ntuple_for_items(items, static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x, static_cast<uint64_t>(gridDim.x) * kBlock, f);
}

// TD: 8T adds per item; an item whose step is 0 loads no board and issues none.  Over plain boards this kernel had no loop
// once and ran 8 waves/SIMD.  The loop keeps the 8T cell lists live across its back edge; left alone the allocator takes
// 106 SGPRs for them, which is 7 waves.  kUpdateMinWaves holds that form to the 8 it had -- the lists beyond 78 SGPRs go to
// VGPR lanes -- and leaves the trace form, which had the loop and 7 waves, as it was
// (profiles/r16_ntuple_items_resource_usage.txt).
template <class Items> constexpr uint32_t kUpdateMinWaves = std::is_same<Items, NtupleBoardItems>::value ? 8u : 1u;

template <uint32_t T, class Shape, class Items>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kUpdateMinWaves<Items>)))
ntuple_update_kernel(const Items items, const int64_t *__restrict__ delta, uint32_t lr_shift, const Shape sh, int32_t *weights)
{
    const AtomicAddWeights add{reinterpret_cast<uint32_t *>(weights)};
    lane_items(items, [&](typename Items::Item it) { ntuple_item_update<T>(items, delta, it, lr_shift, sh, add); });
}

// TC phase W: the 8T offsets, then the 16T 8-byte loads of err and mag in flight together, then the rates and steps, then up
// to 8T adds.  err and mag are only read here: phase A adds to them in a launch of its own, so every lane sees the
// accumulators of before the call.  An item whose d is 0 loads and adds nothing.
template <uint32_t T, class Shape, class Items>
__global__ void __launch_bounds__(kBlock) ntuple_tc_weights_kernel(const Items items, const int64_t *__restrict__ delta, uint32_t lr_shift,
                                                                   const Shape sh, int32_t *weights, const int64_t *__restrict__ err,
                                                                   const int64_t *__restrict__ mag)
{
    const AtomicAddWeights add{reinterpret_cast<uint32_t *>(weights)};
    lane_items(items, [&](typename Items::Item it) { ntuple_item_tc_weights<T>(items, delta, it, lr_shift, sh, err, mag, add); });
}

// TC phase A: 16T 64-bit adds for every item with d != 0, the same items as phase W.
template <uint32_t T, class Shape, class Items>
__global__ void __launch_bounds__(kBlock) ntuple_tc_accum_kernel(const Items items, const int64_t *__restrict__ delta, const Shape sh,
                                                                 int64_t *err, int64_t *mag)
{
    const AtomicAddAccum add{reinterpret_cast<unsigned long long *>(err), reinterpret_cast<unsigned long long *>(mag)};
    lane_items(items, [&](typename Items::Item it) { ntuple_item_tc_accum<T>(items, delta, it, sh, add); });
}

// The batch-mean update (g2048_ntuple_mean_update_plain, g2048_ntuple_mean_trace_update; g2048_device.h "Batch-mean update"):
// two kernels, a launch each, over board or trace items.  All atomics are relaxed and agent scope.  SUM's adds return nothing.
// APPLY's exchanges return the old value: the first reach of an entry to arrive reads count != 0 and owns the entry, every
// other reads the 0 it left.  sum is taken with an exchange too, not a load and a store: an atomic is performed at L2, so
// nothing rests on what a cache of this XCD holds of another XCD's adds, and the array is zero again without a second pass.
struct AtomicAddMean { // sum[off] += d, wrapping mod 2^64; count[off] += 1, wrapping mod 2^32
    unsigned long long *sum;
    uint32_t *count;
    __device__ void operator()(uint32_t off, int64_t d) const
    {
        __hip_atomic_fetch_add(sum + off, static_cast<unsigned long long>(d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(count + off, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct AtomicClaimCount { // exchange(count[off], 0)
    uint32_t *count;
    __device__ uint32_t operator()(uint32_t off) const
    {
        return __hip_atomic_exchange(count + off, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct AtomicTakeSum { // exchange(sum[off], 0)
    unsigned long long *sum;
    __device__ int64_t operator()(uint32_t off) const
    {
        return static_cast<int64_t>(__hip_atomic_exchange(sum + off, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
};

// Phase SUM: 8T 64-bit and 8T 32-bit adds for every item with d != 0.
template <uint32_t T, class Shape, class Items>
__global__ void __launch_bounds__(kBlock) ntuple_mean_sum_kernel(const Items items, const int64_t *__restrict__ delta, const Shape sh,
                                                                 int64_t *sum, uint32_t *count)
{
    const AtomicAddMean add{reinterpret_cast<unsigned long long *>(sum), count};
    lane_items(items, [&](typename Items::Item it) { ntuple_item_mean_sum<T>(items, delta, it, sh, add); });
}

// Phase APPLY: the 8T offsets, the 8T exchanges on count in flight together, then per entry this lane owns one exchange on
// sum, one 64-bit division and one add -- once per distinct reached entry of the call, not once per reach.
template <uint32_t T, class Shape, class Items>
__global__ void __launch_bounds__(kBlock) ntuple_mean_apply_kernel(const Items items, const int64_t *__restrict__ delta, uint32_t lr_shift,
                                                                   const Shape sh, int32_t *weights, int64_t *sum, uint32_t *count)
{
    const AtomicAddWeights add{reinterpret_cast<uint32_t *>(weights)};
    const AtomicClaimCount claim{count};
    const AtomicTakeSum take{reinterpret_cast<unsigned long long *>(sum)};
    lane_items(items, [&](typename Items::Item it) { ntuple_item_mean_apply<T>(items, delta, it, lr_shift, sh, claim, take, add); });
}

// g2048_ntuple_trace_push (the definition of g2048_device.h, "n-tuple traces"): one board per lane -- one 16-byte load of
// the afterstate and one 16-byte store into the slot, the len byte, and delta formed in the same pass (what td_evaluate
// forms with three element-wise launches).  `slot_boards` is the slot's base, hist + slot * n, formed in 64 bits by the
// launcher.  Lanes stride over the boards when n exceeds the grid cap (kSearchMaxLanes).
__global__ void __launch_bounds__(kBlock) ntuple_trace_push_kernel(const uint4 *__restrict__ after,
                                                                   const int64_t *__restrict__ after_value,
                                                                   const int64_t *__restrict__ best_next,
                                                                   const uint8_t *__restrict__ terminated, uint32_t n, uint32_t H,
                                                                   uint4 *__restrict__ slot_boards, uint8_t *__restrict__ len,
                                                                   int64_t *__restrict__ delta)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        const bool term = terminated[i] != 0;
        store_board(slot_boards, static_cast<uint32_t>(i), load_board(after, static_cast<uint32_t>(i)));
        delta[i] = ntuple_trace_delta(best_next[i], after_value[i], term);
        len[i] = static_cast<uint8_t>(ntuple_trace_push_len(len[i], H, term));
    }
}

// g2048_ntuple_delay_push (the definition of g2048_device.h, "n-tuple delay"): ntuple_trace_push_kernel plus the accumulator
// pass, one board per lane, striding past the grid cap.  A lane reads and writes only its own board's accumulators -- up to
// H - 1 8-byte loads issued together, then as many stores, one per plane, each coalesced over the wave -- so there are no
// atomics here.  `acc` is the base of plane 0; the plane base plane * n is formed in 64 bits.
__global__ void __launch_bounds__(kBlock) ntuple_delay_push_kernel(const uint4 *__restrict__ after,
                                                                   const int64_t *__restrict__ after_value,
                                                                   const int64_t *__restrict__ best_next,
                                                                   const uint8_t *__restrict__ terminated, uint32_t n, uint32_t H,
                                                                   uint32_t lam, uint32_t slot, uint4 *__restrict__ slot_boards,
                                                                   uint8_t *__restrict__ len, int64_t *__restrict__ acc,
                                                                   int64_t *__restrict__ delta)
{
    const uint32_t stride = gridDim.x * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        store_board(slot_boards, static_cast<uint32_t>(i), load_board(after, static_cast<uint32_t>(i)));
        uint8_t l = len[i];
        delta[i] = ntuple_delay_push(l, best_next[i], after_value[i], terminated[i] != 0, lam, slot, H,
                                     [&](uint32_t plane) -> int64_t & { return acc[static_cast<uint64_t>(plane) * n + i]; });
        len[i] = l;
    }
}

// ---------------------------------------------------------------------------- carousel shaping
// g2048_carousel_step (the definition of g2048_device.h, "carousel shaping") is three launches on one stream; the launch
// boundaries are the only synchronisation between workgroups -- no kernel here waits for another workgroup in any form.
// Workgroup w takes the boards [w * per, (w + 1) * per) (carousel_range: at most kCarouselMaxGroups workgroups, whatever n),
// in chunks of kBlock, so that ascending board index is the order of (workgroup, chunk, wave, lane).
//   restart  per board: one 16-byte load; a terminated board reads episodes, count and the pool and stores the restarted
//            record; a board that goes on computes its stage and updates seen, marking an entry with kCarouselEntryBit.  The
//            pool and count are only read here, so every lane sees them as they were before the call.  Every workgroup
//            leaves its entry count per stage in cnt[k][w].
//   scan     one workgroup: prefix[k][w] = cnt[k][0] + .. + cnt[k][w-1], total[k], count_mod[k] = count[k] mod C, and then
//            count[k] += total[k].
//   scatter  a workgroup with entries reads seen again, clears the marks, recomputes every entry's rank -- prefix[k][w],
//            the entries of the chunks and waves before it (LDS), the lanes before it (ballot) -- and stores the surviving
//            records into the pool.  A call without entries, and a workgroup without, leaves at once.
// Scratch (uint32): cnt[8][kCarouselMaxGroups] | prefix[8][kCarouselMaxGroups] | total[8] | count_mod[8].
static_assert(kCarouselMaxGroups == 4u * kBlock, "carousel_scan_kernel scans four workgroup counts per lane");
static_assert(kCarouselScratchBytes == (16u * kCarouselMaxGroups + 16u) * sizeof(uint32_t), "the carousel's scratch layout");
constexpr uint32_t kCarouselWaves = kBlock / 64;

struct CarouselParams {
    uint4 *records;
    const uint8_t *terminated;
    uint4 *pool;
    uint64_t *count;
    uint8_t *seen;
    uint32_t *episodes;
    uint32_t *scratch;
    CarouselStages cs;
    uint32_t n, index_offset, n_stages, capacity, seed_lo, seed_hi;
    uint64_t per; // boards per workgroup
};

__device__ __forceinline__ uint32_t *carousel_cnt(const CarouselParams &p, uint32_t k) { return p.scratch + k * kCarouselMaxGroups; }
__device__ __forceinline__ uint32_t *carousel_prefix(const CarouselParams &p, uint32_t k)
{
    return p.scratch + (kNtupleMaxStages + k) * kCarouselMaxGroups;
}
__device__ __forceinline__ uint32_t *carousel_total(const CarouselParams &p) { return p.scratch + 2u * kNtupleMaxStages * kCarouselMaxGroups; }
__device__ __forceinline__ uint32_t *carousel_count_mods(const CarouselParams &p) { return carousel_total(p) + kNtupleMaxStages; }

// the set bits of a ballot below this lane
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

__global__ void __launch_bounds__(kBlock) carousel_restart_kernel(const CarouselParams p)
{
    __shared__ uint32_t s_cnt[kCarouselWaves][kNtupleMaxStages];
    const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
    const uint64_t begin = blockIdx.x * p.per, end = begin + p.per < p.n ? begin + p.per : p.n;
    const uint32_t top = carousel_top_stage(p.count, p.n_stages);
    uint32_t wave_cnt[kNtupleMaxStages] = {}; // wave-uniform, statically indexed
    for (uint64_t base = begin; base < end; base += kBlock) {
        bool entry = false;
        uint32_t st = 0;
        if (base + threadIdx.x < end) {
            const uint32_t i = static_cast<uint32_t>(base + threadIdx.x);
            const Board rec = load_board(p.records, i);
            if (p.terminated[i] != 0) {
                const uint32_t e = p.episodes[i];
                p.episodes[i] = e + 1u;
                const uint32_t g = p.index_offset + i;
                const uint32_t k = carousel_stage_choice(g, e, top);
                const uint64_t made = k > 0u ? p.count[k] : 0ull;
                uint32_t seen;
                if (made > 0ull) {
                    const uint32_t j = carousel_sample(e, g, k, carousel_fill(made, p.capacity), p.seed_lo, p.seed_hi);
                    store_board(p.records, i, load_board(p.pool, k * p.capacity + j));
                    seen = k;
                } else {
                    seen = carousel_stage(rec, p.cs);
                }
                p.seen[i] = static_cast<uint8_t>(seen);
            } else {
                st = carousel_stage(rec, p.cs);
                const uint32_t old = p.seen[i], next = carousel_seen_next(old, st);
                entry = next != old && (next & kCarouselEntryBit) != 0u;
                if (next != old)
                    p.seen[i] = static_cast<uint8_t>(next);
            }
        }
        if (g2048_any(entry)) {
#pragma unroll
            for (uint32_t k = 1; k < kNtupleMaxStages; ++k)
                wave_cnt[k] += static_cast<uint32_t>(__popcll(__builtin_amdgcn_ballot_w64(entry && st == k)));
        }
    }
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < kNtupleMaxStages; ++k)
            s_cnt[wave][k] = wave_cnt[k];
    }
    __syncthreads();
    if (threadIdx.x < kNtupleMaxStages) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kCarouselWaves; ++w)
            sum += s_cnt[w][threadIdx.x];
        carousel_cnt(p, threadIdx.x)[blockIdx.x] = sum;
    }
}

__global__ void __launch_bounds__(kBlock) carousel_scan_kernel(const CarouselParams p, uint32_t groups)
{
    __shared__ uint32_t s_wave[kCarouselWaves];
    const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
    for (uint32_t k = 1; k < p.n_stages; ++k) {
        const uint32_t *cnt = carousel_cnt(p, k);
        uint32_t *prefix = carousel_prefix(p, k);
        uint32_t v[4], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t w = 4u * threadIdx.x + j;
            v[j] = w < groups ? cnt[w] : 0u; // (the scratch beyond `groups` is not this call's)
            sum += v[j];
        }
        uint32_t incl = sum; // inclusive scan over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            incl += lane >= d ? up : 0u;
        }
        if (lane == 63u)
            s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kCarouselWaves; ++w) {
            before += w < wave ? s_wave[w] : 0u;
            total += s_wave[w];
        }
        uint32_t run = before + incl - sum;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t w = 4u * threadIdx.x + j;
            if (w < groups)
                prefix[w] = run;
            run += v[j];
        }
        if (threadIdx.x == 0u) {
            const uint64_t made = p.count[k];
            carousel_total(p)[k] = total;
            carousel_count_mods(p)[k] = carousel_count_mod(made, p.capacity);
            p.count[k] = made + total;
        }
        __syncthreads(); // s_wave is written again for the next stage
    }
}

__global__ void __launch_bounds__(kBlock) carousel_scatter_kernel(const CarouselParams p)
{
    __shared__ uint32_t s_wave[kCarouselWaves][kNtupleMaxStages]; // the entries of each wave in this chunk
    __shared__ uint32_t s_base[kNtupleMaxStages];                 // the entries before this chunk
    const uint32_t *total = carousel_total(p), *count_mod = carousel_count_mods(p);
    uint32_t any = 0, mine = 0;
    for (uint32_t k = 1; k < p.n_stages; ++k) {
        any |= total[k];
        mine |= carousel_cnt(p, k)[blockIdx.x];
    }
    if (any == 0u || mine == 0u)
        return; // (uniform over the workgroup: nobody is left at a barrier)
    const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
    const uint64_t begin = blockIdx.x * p.per, end = begin + p.per < p.n ? begin + p.per : p.n;
    // lane k < 8 carries the running base of stage k
    uint32_t base_k = threadIdx.x >= 1u && threadIdx.x < p.n_stages ? carousel_prefix(p, threadIdx.x)[blockIdx.x] : 0u;
    for (uint64_t base = begin; base < end; base += kBlock) {
        const bool live = base + threadIdx.x < end;
        const uint32_t i = static_cast<uint32_t>(base + threadIdx.x);
        const uint32_t seen = live ? p.seen[i] : kCarouselUnknown;
        const bool entry = carousel_is_entry(seen);
        const uint32_t st = seen & (kNtupleMaxStages - 1u);
        uint32_t below = 0;
#pragma unroll
        for (uint32_t k = 1; k < kNtupleMaxStages; ++k) {
            const uint64_t mask = __builtin_amdgcn_ballot_w64(entry && st == k);
            below = st == k ? lanes_below(mask) : below;
            if (lane == 0u)
                s_wave[wave][k] = static_cast<uint32_t>(__popcll(mask));
        }
        if (threadIdx.x < kNtupleMaxStages)
            s_base[threadIdx.x] = base_k;
        __syncthreads();
        if (entry) {
            uint32_t r = s_base[st] + below;
            for (uint32_t w = 0; w < wave; ++w)
                r += s_wave[w][st];
            p.seen[i] = static_cast<uint8_t>(st);
            // (st >= 1 and st < S for every mark the restart pass made; the test keeps any other byte inside the pool)
            if (st >= 1u && st < p.n_stages && carousel_survives(r, total[st], p.capacity))
                store_board(p.pool, st * p.capacity + carousel_slot(count_mod[st], r, p.capacity), load_board(p.records, i));
        }
        if (threadIdx.x >= 1u && threadIdx.x < kNtupleMaxStages) {
            for (uint32_t w = 0; w < kCarouselWaves; ++w)
                base_k += s_wave[w][threadIdx.x];
        }
        __syncthreads(); // s_wave and s_base are written again for the next chunk
    }
}

// ---------------------------------------------------------------------------- augmentation
// training_data.augment() (training_data.py:257-299) for board pairs on the device: the eight
// symmetries [orig, hflip, rot1(orig), rot1(hflip), rot2(..), rot2(..), rot3(..), rot3(..)] with the
// action remapped (hflip swaps 1 <-> 3, :262-267; a clockwise quarter turn adds 1 mod 4, :276).
// One lane per (variant, transition); every access is a coalesced 16-byte load/store.
__device__ __forceinline__ Board hflip_board(const Board &b) // np.flip(x, 2): reverse every row
{
    return Board{{__builtin_bswap32(b.r[0]), __builtin_bswap32(b.r[1]), __builtin_bswap32(b.r[2]), __builtin_bswap32(b.r[3])}};
}

__device__ __forceinline__ Board rotate_board(const Board &b, uint32_t k) // np.rot90(x, k, axes=(2, 1)): clockwise
{
    const Board t = transpose(b);
    if (k == 1u) // out[r][c] = in[3-c][r]
        return Board{{__builtin_bswap32(t.r[0]), __builtin_bswap32(t.r[1]), __builtin_bswap32(t.r[2]), __builtin_bswap32(t.r[3])}};
    if (k == 2u) // out[r][c] = in[3-r][3-c]
        return Board{{__builtin_bswap32(b.r[3]), __builtin_bswap32(b.r[2]), __builtin_bswap32(b.r[1]), __builtin_bswap32(b.r[0])}};
    if (k == 3u) // out[r][c] = in[c][3-r]
        return Board{{t.r[3], t.r[2], t.r[1], t.r[0]}};
    return b;
}

__global__ void __launch_bounds__(kBlock) augment_kernel(const uint4 *__restrict__ boards, const uint4 *__restrict__ next_boards,
                                                         const uint8_t *__restrict__ actions, uint32_t n,
                                                         uint4 *__restrict__ boards_out, uint4 *__restrict__ next_out,
                                                         uint8_t *__restrict__ actions_out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t variant = blockIdx.y; // 0..7
    if (i >= n)
        return;
    const uint32_t flip = variant & 1u, k = variant >> 1;
    uint4 v = boards[i];
    Board b{{v.x, v.y, v.z, v.w}};
    uint32_t a = actions[i];
    if (flip) {
        b = hflip_board(b);
        a = (a == 1u) ? 3u : (a == 3u ? 1u : a);
    }
    b = rotate_board(b, k);
    a = (a + k) & 3u;
    const size_t o = static_cast<size_t>(variant) * n + i;
    boards_out[o] = make_uint4(b.r[0], b.r[1], b.r[2], b.r[3]);
    actions_out[o] = static_cast<uint8_t>(a);
    if (next_boards) {
        v = next_boards[i];
        Board nb{{v.x, v.y, v.z, v.w}};
        if (flip)
            nb = hflip_board(nb);
        nb = rotate_board(nb, k);
        next_out[o] = make_uint4(nb.r[0], nb.r[1], nb.r[2], nb.r[3]);
    }
}

// ------------------------------------------------------------------------- canonicalisation
// Symmetric-board canonicalisation: of the eight symmetries training_data.augment()
// generates (training_data.py:257-299, same order: variant = 2 * quarter_turns + hflip), keep the one
// whose 16 cells, read row-major as bytes, are lexicographically smallest (ties: the lowest variant
// index); the action is remapped and the next board transformed by the same symmetry.  In place.
// Row-major byte order = compare r[0] first, byte 0 most significant: bswap makes that an integer compare.
__device__ __forceinline__ bool board_less(const Board &a, const Board &b)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x = __builtin_bswap32(a.r[k]), y = __builtin_bswap32(b.r[k]);
        if (x != y)
            return x < y;
    }
    return false;
}

__device__ __forceinline__ Board symmetry(const Board &b, uint32_t variant)
{
    return rotate_board((variant & 1u) ? hflip_board(b) : b, variant >> 1);
}

__global__ void __launch_bounds__(kBlock) canonicalize_kernel(uint4 *boards, uint4 *next_boards, uint8_t *actions,
                                                              uint32_t n, uint8_t *sym_out)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const Board b = load_board(boards, i);
    Board best = b;
    uint32_t best_v = 0;
#pragma unroll
    for (uint32_t v = 1; v < 8; ++v) {
        const Board c = symmetry(b, v);
        if (board_less(c, best)) {
            best = c;
            best_v = v;
        }
    }
    store_board(boards, i, best);
    if (next_boards)
        store_board(next_boards, i, symmetry(load_board(next_boards, i), best_v));
    if (actions) {
        uint32_t a = actions[i] & 3u;
        if (best_v & 1u)
            a = (a == 1u) ? 3u : (a == 3u ? 1u : a); // hflip swaps right <-> left (:262-267)
        actions[i] = static_cast<uint8_t>((a + (best_v >> 1)) & 3u); // a clockwise quarter turn adds 1 (:276)
    }
    if (sym_out)
        sym_out[i] = static_cast<uint8_t>(best_v);
}

// ----------------------------------------------------------------------------------- stats
// Reduce to one StatsOut: the episode counters, the exact sum of the final scores of ALL finished episodes
// (return_sum = sum of the slots' G - sum of the scores of the boards whose episode is still running, see the slot
// layout above), the returns of the boards' most recent finished episodes (score of last_record: count / sum / max),
// the highest tile on any board and the histogram of the boards' highest tiles (what ppo_train.py:77-81 tallies per
// finished episode, here for the live boards).  Two stages and NO global atomics: a single hot cache line serialises at
// ~88 atomics/us on this chip (a one-stage version spent 55 us at 2^20 boards in its ~5 000 final atomics).
//   stage 1: every block reduces its grid-stride share (registers, then a tree in LDS) to kStatsFields
//            numbers, stored field-major: partials[f * kStatsBlocks + block].  The histogram is counted by
//            per-wave ballots (the counts are wave-uniform: they live in SGPRs);
//   stage 2: kStatsFields blocks, block f reduces field f over the partials (coalesced reads, tree in LDS).
// Cross-lane shuffles are avoided on purpose: a 64-bit __shfl_xor chain costs ~100 cycles per step and the
// reductions here are latency-, not throughput-bound.
constexpr int kStatsScalars = 7; // episodes, illegal_ends, last_count, last_score_sum, last_score_max, max_exp, return_sum
constexpr int kStatsFields = kStatsScalars + 32; // + hist[32]
static_assert(kStatsFields * kStatsBlocks == kStatsPartialWords, "partials buffer size");

// (The RETURNS-ONLY flavour -- what a multi-GPU job all-gathers once per rollout -- is returns_summary_kernel below: one
// launch.  Until round 6 it was this kernel pair without the terminal records and the histogram: 11.5 us per call at 2^20
// boards against 7.4, profiles/r06_b_stats_probe_*.txt.)
__global__ void __launch_bounds__(kBlock) stats_kernel(const DeviceState st, uint32_t n, uint32_t n_waves,
                                                       unsigned long long *partials)
{
    __shared__ unsigned long long s_ep[kBlock], s_ill[kBlock], s_sum[kBlock], s_cnt[kBlock], s_ret[kBlock];
    __shared__ unsigned int s_max[kBlock], s_exp[kBlock];
    __shared__ unsigned int s_hist[32];
    unsigned long long episodes = 0, illegal = 0, score_sum = 0, count = 0;
    unsigned long long ret = 0; // sum of G over this thread's slots - sum of the live scores of its boards (mod 2^64)
    unsigned int max_score = 0, max_exp = 0;
    uint32_t hist[32];
#pragma unroll
    for (int b = 0; b < 32; ++b)
        hist[b] = 0u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < 32u)
        s_hist[tid] = 0u;
    __syncthreads();
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t wv = blockIdx.x * kBlock + tid; wv < n_waves; wv += stride) {
        const uint32_t *slot = slot_of(st.ep_counters, wv);
        const uint4 lo = *reinterpret_cast<const uint4 *>(slot), hi = *reinterpret_cast<const uint4 *>(slot + 4);
        episodes += static_cast<unsigned long long>(hi.x) << 32 | lo.x;
        illegal += static_cast<unsigned long long>(hi.y) << 32 | lo.y;
        ret += static_cast<unsigned long long>(hi.z) << 32 | lo.z;
    }
    // whole wavefronts iterate together (the ballots need every lane's vote): lanes past the end vote "none"
    for (uint64_t base = blockIdx.x * kBlock + tid - lane; base < n; base += stride) { // 64-bit: n may be near 2^32
        const uint64_t i = base + lane;
        // boards whose episode has ended but which were not reset (auto_reset == 0): their score is a finished episode's
        const unsigned long long pending = slot_get(slot_of(st.ep_counters, static_cast<uint32_t>(base >> 6)), kSlotPending); // uniform: scalar loads
        uint32_t h = 0xffu;
        if (i < n) {
            const Board live = load_board_nt(st.boards, static_cast<uint32_t>(i));
            if (((pending >> lane) & 1ull) == 0ull)
                ret -= record_score(live);
            h = highest(record_cells(live));
            max_exp = max(max_exp, h);
            Board last{{0u, 0u, 0u, 0u}};
            if (st.last_record) // NULL: terminal records are not kept, last_* stay zero
                last = load_board_nt(st.last_record, static_cast<uint32_t>(i));
            if ((last.r[0] | last.r[1] | last.r[2] | last.r[3]) != 0u) { // a terminal board is never empty
                const unsigned int sc = record_score(last);
                count += 1;
                score_sum += sc;
                max_score = max(max_score, sc);
            }
        }
#pragma unroll
        for (uint32_t b = 0; b < 32u; ++b)
            hist[b] += static_cast<uint32_t>(__popcll(__builtin_amdgcn_ballot_w64(h == b)));
    }
    s_ep[tid] = episodes; s_ill[tid] = illegal; s_sum[tid] = score_sum; s_cnt[tid] = count; s_ret[tid] = ret;
    s_max[tid] = max_score; s_exp[tid] = max_exp;
    if (lane == 0u) {
#pragma unroll
        for (int b = 0; b < 32; ++b)
            if (hist[b] != 0u)
                atomicAdd(&s_hist[b], hist[b]);
    }
    __syncthreads();
    for (uint32_t off = kBlock / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_ep[tid] += s_ep[tid + off];
            s_ill[tid] += s_ill[tid + off];
            s_sum[tid] += s_sum[tid + off];
            s_cnt[tid] += s_cnt[tid + off];
            s_ret[tid] += s_ret[tid + off];
            s_max[tid] = max(s_max[tid], s_max[tid + off]);
            s_exp[tid] = max(s_exp[tid], s_exp[tid + off]);
        }
        __syncthreads();
    }
    unsigned long long *mine = partials + blockIdx.x;
    if (tid == 0) {
        mine[0 * kStatsBlocks] = s_ep[0];
        mine[1 * kStatsBlocks] = s_ill[0];
        mine[2 * kStatsBlocks] = s_cnt[0];
        mine[3 * kStatsBlocks] = s_sum[0];
        mine[4 * kStatsBlocks] = s_max[0];
        mine[5 * kStatsBlocks] = s_exp[0];
        mine[6 * kStatsBlocks] = s_ret[0];
    }
    if (tid < 32u)
        mine[(kStatsScalars + tid) * kStatsBlocks] = s_hist[tid];
}

// block f: field f of every partial -> the matching member of *out (fields 4 and 5 are maxima, the rest sums mod 2^64)
// last_known: the terminal records were read (the full flavour on an engine that keeps them).  Otherwise last_count and
// last_score_sum are 0 and last_score_max is -1 -- "not computed", which no score can be -- so that a reader of the struct
// (parse_stats, a peer rank behind an all-gather) cannot mistake the zeros for a measured mean of 0.
__global__ void __launch_bounds__(kBlock) stats_merge_kernel(const unsigned long long *partials, uint32_t n_partials,
                                                             StatsOut *out, bool last_known)
{
    __shared__ unsigned long long s_v[kBlock];
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const bool is_max = f == 4u || f == 5u;
    unsigned long long v = 0;
    for (uint32_t q = tid; q < n_partials; q += kBlock) {
        const unsigned long long x = partials[f * kStatsBlocks + q];
        v = is_max ? (x > v ? x : v) : v + x;
    }
    s_v[tid] = v;
    __syncthreads();
    for (uint32_t off = kBlock / 2; off > 0; off >>= 1) {
        if (tid < off) {
            const unsigned long long a = s_v[tid], b = s_v[tid + off];
            s_v[tid] = is_max ? (b > a ? b : a) : a + b;
        }
        __syncthreads();
    }
    if (tid != 0)
        return;
    v = s_v[0];
    switch (f) {
    case 0: out->episodes = v; break;
    case 1: out->illegal_ends = v; break;
    case 2: out->last_count = v; break;
    case 3: out->last_score_sum = v; break;
    case 4: out->last_score_max = last_known ? static_cast<int>(v) : -1; break;
    case 5: out->max_exp = static_cast<unsigned int>(v); break;
    case 6: out->return_sum = static_cast<long long>(v); break;
    default: out->highest_hist[f - kStatsScalars] = static_cast<unsigned int>(v); break;
    }
}

// ------------------------------------------------------------- the returns summary in ONE launch
// What the once-per-rollout exchange of a multi-GPU job ships (first option): episodes, illegal_ends and the
// exact return_sum, from the episode slots and the live records -- the returns-only flavour of the reduction above, which
// as a kernel PAIR cost 11-13 us at 2^20 boards behind the last step of a rollout (two launches, a 2 048-column partials
// buffer in between).  Here: at most kSummaryBlocks blocks of 1 024 lanes (one per CU, sixteen wavefronts each), every
// wavefront walks whole 64-board groups = whole slots (slot through the scalar cache, the pending mask with it; four
// record loads in flight per lane), and the merge happens in the SAME launch by "last one out".
//
// Every word that crosses a block boundary travels by a device-scope read-modify-write and nothing else: a block PUBLISHES
// its three sums with atomic exchanges into its own 32-byte partial, waits for their return values (an RMW returns after it
// has been performed at the point of coherence -- the partial of a block on another XCD never sits in that XCD's L2), then
// counts itself in.  Counting is two-level -- one counter per group of kSummaryGroup blocks and one for the groups, each on
// its own cache line -- because a single hot line serialises at ~88 atomics/us on this chip (256 arrivals on one line:
// up to 2.9 us; 16: 0.2).  The block that finds itself last of the last group READS the partials back with RMWs as well
// (one lane per block, all in flight together), so there is no cache write-back or invalidate on the path at all (an
// agent-scope fence on gfx950 is a buffer_wbl2 + buffer_inv of the whole L2: the first version of this kernel, with three
// fence pairs and one lane walking the partials, took 15.8 us at 2^20 boards against 11.6 for the kernel pair,
// profiles/r06_a_stats_probe_*.txt).  The counters are left at zero for the next launch (calls on one engine are
// stream-ordered).
constexpr uint32_t kSummaryThreads = 1024, kSummaryGroup = 16;
constexpr uint32_t kSummaryGroups = kSummaryBlocks / kSummaryGroup;
constexpr uint32_t kSumCounterBase = kSummaryBlocks * 4;   // uint64 words: the block partials, then the counters (one 64-byte line each)
static_assert(kSumCounterBase + (kSummaryGroups + 1) * 8 <= kSummaryScratchWords, "summary scratch size");
static_assert(kSummaryBlocks % kSummaryGroup == 0 && kSummaryBlocks <= kSummaryThreads, "whole groups; one lane per partial");

// sum over the 16 cells of (e - 1) * 2^e as three instructions per cell: an empty cell contributes (0 - 1) << 0 = -1,
// put back by count_empty.  (g2048_device.h potential() keeps two sums: five instructions per cell.)
__device__ __forceinline__ uint32_t potential_lean(const Board &cells)
{
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const uint32_t e = (cells.r[i] >> (8 * l)) & 0xffu;
            acc += (e - 1u) << (e & 31u);
        }
    }
    return acc + count_empty(cells);
}

__device__ __forceinline__ uint32_t record_score_lean(const Board &raw)
{
    return (potential_lean(record_cells(raw)) - record_deficit(raw)) & kScoreMask;
}

__device__ __forceinline__ unsigned long long rmw_exchange(unsigned long long *p, unsigned long long v)
{
    return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a READ as a read-modify-write: `zero` is 0 in a form the compiler cannot see through (it would turn an add of a
// literal 0 into a plain sc1 load, which an L2 is allowed to serve)
__device__ __forceinline__ unsigned long long rmw_read(unsigned long long *p, unsigned long long zero)
{
    return __hip_atomic_fetch_add(p, zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the value has arrived (s_waitcnt) before anything behind this point is issued
__device__ __forceinline__ void wait_for(unsigned long long v) { asm volatile("" ::"v"(v) : "memory"); }

__global__ void __launch_bounds__(kSummaryThreads) returns_summary_kernel(const DeviceState st, uint32_t n, uint32_t n_waves,
                                                                          unsigned long long *scratch, StatsOut *out)
{
    constexpr uint32_t kWaves = kSummaryThreads / 64u, kUnroll = 4u;
    __shared__ unsigned long long s_part[kWaves][3];
    __shared__ uint32_t s_last;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t wave_stride = gridDim.x * kWaves;
    unsigned long long episodes = 0, illegal = 0, gain = 0; // wave-uniform: the slots' counters
    unsigned long long live = 0;                            // this lane's share of the scores of the RUNNING episodes
    for (uint32_t w0 = blockIdx.x * kWaves + wave_in_block; w0 < n_waves; w0 += kUnroll * wave_stride) {
        Board rec[kUnroll];
        bool counts[kUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const uint32_t w = w0 + u * wave_stride;
            const bool have = w < n_waves;                  // uniform
            const uint32_t wc = have ? w : w0;
            const uint32_t *slot = slot_of(st.ep_counters, wc);
            const uint4 lo = *reinterpret_cast<const uint4 *>(slot), hi = *reinterpret_cast<const uint4 *>(slot + 4);
            if (have) {
                episodes += static_cast<unsigned long long>(hi.x) << 32 | lo.x;
                illegal += static_cast<unsigned long long>(hi.y) << 32 | lo.y;
                gain += static_cast<unsigned long long>(hi.z) << 32 | lo.z;
            }
            // a board whose episode has ended but which was not reset (auto_reset == 0) holds a FINISHED episode's score
            const unsigned long long pending = static_cast<unsigned long long>(hi.w) << 32 | lo.w;
            const uint64_t i = static_cast<uint64_t>(wc) * 64u + lane;
            counts[u] = have && i < n && ((pending >> lane) & 1ull) == 0ull;
            rec[u] = load_board_nt(st.boards, static_cast<uint32_t>(i < n ? i : n - 1u));
        }
#pragma unroll
        for (uint32_t u = 0; u < kUnroll; ++u)
            live += counts[u] ? record_score_lean(rec[u]) : 0u;
    }
    const unsigned long long live_wave = wave_sum64_lane63(live); // (every lane is here: the loop bounds are uniform)
    if (lane == 63u) {
        s_part[wave_in_block][0] = episodes;
        s_part[wave_in_block][1] = illegal;
        s_part[wave_in_block][2] = gain - live_wave;            // mod 2^64
    }
    __syncthreads();
    const uint32_t blocks = gridDim.x;
    if (tid == 0u) {
        unsigned long long ep = 0, ill = 0, ret = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            ep += s_part[w][0];
            ill += s_part[w][1];
            ret += s_part[w][2];
        }
        uint32_t last = 0u;
        if (blocks == 1u) { // nothing to merge: wave 0 below reads these back from LDS
            s_part[0][0] = ep;
            s_part[0][1] = ill;
            s_part[0][2] = ret;
            last = 2u;
        } else {
            unsigned long long *mine = scratch + 4u * blockIdx.x;
            const unsigned long long r0 = rmw_exchange(mine + 0, ep), r1 = rmw_exchange(mine + 1, ill), r2 = rmw_exchange(mine + 2, ret);
            wait_for(r0 | r1 | r2);                             // published (performed at the point of coherence) ...
            const uint32_t group = blockIdx.x / kSummaryGroup, groups = (blocks + kSummaryGroup - 1u) / kSummaryGroup;
            const uint32_t members = min(kSummaryGroup, blocks - group * kSummaryGroup);
            unsigned int *group_count = reinterpret_cast<unsigned int *>(scratch + kSumCounterBase + 8u * group);
            unsigned int *top_count = reinterpret_cast<unsigned int *>(scratch + kSumCounterBase + 8u * kSummaryGroups);
            if (atomicAdd(group_count, 1u) == members - 1u) {   // ... before this block counts itself in
                atomicExch(group_count, 0u);                    // (nobody else touches it again in this launch)
                if (atomicAdd(top_count, 1u) == groups - 1u) {
                    atomicExch(top_count, 0u);
                    last = 1u;
                }
            }
        }
        s_last = last;
    }
    __syncthreads();
    const uint32_t last = s_last;                               // block-uniform
    if (last == 0u || tid >= 64u)
        return;
    // the last block out: lane b of wavefront 0 ... reads partial b, b + 64, ... (all RMWs in flight together)
    unsigned long long ep = 0, ill = 0, ret = 0;
    if (last == 2u) {
        if (lane == 0u) {
            ep = s_part[0][0];
            ill = s_part[0][1];
            ret = s_part[0][2];
        }
    } else {
        unsigned long long v[3 * (kSummaryBlocks / 64u)];
#pragma unroll
        for (uint32_t q = 0; q < kSummaryBlocks / 64u; ++q) {
            const uint32_t b = q * 64u + lane;
            unsigned long long *theirs = scratch + 4u * (b < blocks ? b : 0u);
#pragma unroll
            for (uint32_t f = 0; f < 3u; ++f)
                v[3u * q + f] = b < blocks ? rmw_read(theirs + f, last >> 8) : 0ull; // (last is 1 here)
        }
#pragma unroll
        for (uint32_t q = 0; q < kSummaryBlocks / 64u; ++q) {
            ep += v[3u * q + 0];
            ill += v[3u * q + 1];
            ret += v[3u * q + 2];
        }
    }
    ep = wave_sum64_lane63(ep);
    ill = wave_sum64_lane63(ill);
    ret = wave_sum64_lane63(ret); // (a sum mod 2^64: a block's gain - live may be "negative")
    if (lane != 63u)
        return;
    // the terminal records were not read and nothing was counted for the histogram: "not computed" (last_score_max = -1,
    // which no score can be), so that a reader of the struct cannot mistake the zeros for a measured mean of 0
    out->episodes = ep;
    out->illegal_ends = ill;
    out->last_count = 0;
    out->last_score_sum = 0;
    out->last_score_max = -1;
    out->max_exp = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k)
        out->highest_hist[k] = 0u;
    out->return_sum = static_cast<long long>(ret);
}

// -------------------------------------------------------------------------------- launchers
static inline dim3 grid_for(uint64_t items) { return dim3(static_cast<uint32_t>((items + kBlock - 1) / kBlock)); }

// One lane per item in blocks of kBlock, `lds` bytes of dynamic LDS; nothing to do for n == 0.
template <class... Params, class... Args>
static hipError_t launch_1d(void (*kernel)(Params...), uint64_t n, uint32_t lds, hipStream_t s, Args... args)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(kernel, grid_for(n), dim3(kBlock), lds, s, args...);
    return hipGetLastError();
}

// f(std::integral_constant<int, V>()) for the runtime value v = V in FIRST..LAST (an action dtype, an obs dtype): one
// instantiation of f per value in the range.  Any other v is hipErrorInvalidValue.
template <int FIRST, int LAST, class F>
static hipError_t dispatch(int v, F &&f)
{
    if constexpr (FIRST > LAST)
        return hipErrorInvalidValue;
    else
        return v == FIRST ? f(std::integral_constant<int, FIRST>()) : dispatch<FIRST + 1, LAST>(v, f);
}

// f(std::bool_constant<B>()) for the runtime b = B
template <class F>
static hipError_t dispatch_bool(bool b, F &&f)
{
    return b ? f(std::true_type()) : f(std::false_type());
}

// f(act, std::bool_constant<FULL>()) for the template arguments <ACT, FULL> of the step kernels
template <class F>
static hipError_t dispatch_step(int action_dtype, bool full, F &&f)
{
    return dispatch<0, 3>(action_dtype, [&](auto act) { return dispatch_bool(full, [&](auto full_c) { return f(act, full_c); }); });
}

hipError_t launch_reset(const StepArgs &a, uint32_t first_slot, const uint8_t *mask, hipStream_t s)
{
    if (a.st.rng)
        return launch_1d(reset_numpy_kernel, a.n, 0, s, a, mask);
    return launch_1d(reset_kernel, a.n, 0, s, a, first_slot, mask);
}

// The outputs of step_kernel's STD configuration: reward and terminated, nothing optional, no max tile
static bool standard_outputs(const StepArgs &a)
{
    return a.reward && a.terminated && !a.illegal && !a.highest && !a.terminal_boards && a.max_exp == 0 && !a.boards_out &&
           !a.done_seq;
}

template <int ACT, bool FULL, bool STD, bool OBS>
static void enqueue_step(const StepArgs &a, hipStream_t s)
{
    constexpr auto kernel = step_kernel<ACT, FULL, STD, OBS>;
    uint32_t pad = 0u;
    if constexpr (OBS)
        pad = obs_pad_for<kernel>();
    hipLaunchKernelGGL(kernel, grid_for(a.n), dim3(kBlock), pad, s, a.st.boards, a.actions, a.st.ep_counters, a.board_offset,
                       a.seed_lo, a.seed_hi, a.t_lo, a.t_hi, a.n, a.reward, step_tail(a));
}

hipError_t launch_step(const StepArgs &a, int action_dtype, hipStream_t s)
{
    if (a.n == 0)
        return hipSuccess;
    if (a.st.rng) {
        // numpy-RNG mode: a block's resets run after its steps, so the observation and the plain boards come from the
        // stand-alone kernels behind it
        hipError_t err = dispatch<0, 3>(action_dtype, [&](auto act) {
            hipLaunchKernelGGL(step_numpy_kernel<act>, dim3((a.n + kNumpyBlock - 1u) / kNumpyBlock), dim3(kNumpyBlock), 0, s, a);
            return a.obs ? launch_onehot(a.st.boards, a.n, a.obs, static_cast<int>(a.obs_dtype), s) : hipGetLastError();
        });
        if (err == hipSuccess && a.boards_out)
            err = launch_export_boards(a.st.boards, a.n, a.boards_out, s);
        return err;
    }
    const bool standard = standard_outputs(a) && !(a.action_err && action_dtype != 0);
    const hipError_t known = dispatch_step(action_dtype, a.n % kBlock == 0, [&](auto act, auto full) {
        if (standard && a.obs)
            enqueue_step<act, full, true, true>(a, s);
        else if (standard)
            enqueue_step<act, full, true, false>(a, s);
        else if (a.obs)
            enqueue_step<act, full, false, true>(a, s);
        else
            enqueue_step<act, full, false, false>(a, s);
        return hipSuccess;
    });
    if (known != hipSuccess)
        return known;
    if (a.done_seq && grid_for(a.n).x > 1) // a one-block launch has published the word itself
        hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(64), 0, s, a.done_seq, a.done_value);
    return hipGetLastError();
}

hipError_t launch_move(uint4 *boards, uint32_t n, const void *actions, int action_dtype, bool trial,
                       int32_t *score_out, uint8_t *legal_out, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    const uint32_t tr = trial ? 1u : 0u;
    return dispatch<1, 3>(action_dtype, // (no move_kernel<0>: a move needs an action buffer)
                          [&](auto act) { return launch_1d(move_kernel<act>, n, 0, s, boards, n, actions, tr, score_out, legal_out); });
}

hipError_t launch_query(const uint4 *boards, uint32_t n, uint32_t max_exp, uint8_t *isend_out, uint8_t *highest_out,
                        hipStream_t s)
{
    return launch_1d(query_kernel, n, 0, s, boards, n, max_exp, isend_out, highest_out);
}

hipError_t launch_legal_mask(const uint4 *boards, uint32_t n, uint8_t *mask_out, hipStream_t s)
{
    return launch_1d(legal_mask_kernel, n, 0, s, boards, n, mask_out);
}

hipError_t launch_afterstates(const Boards &b, const AfterstateOut &o, hipStream_t s)
{
    return dispatch_bool(b.plain, [&](auto plain_c) {
        if (o.obs)
            return launch_1d(afterstates_kernel<plain_c, true>, b.n, kAfterstateObsPad, s, b.ptr, b.n, o);
        return launch_1d(afterstates_kernel<plain_c, false>, b.n, 0, s, b.ptr, b.n, o);
    });
}

// Lanes of a launch that gives each of n boards a group of G, up to the grid cap (the groups stride beyond it)
static uint64_t group_lanes(uint32_t n, uint32_t G)
{
    const uint64_t want = static_cast<uint64_t>(n) * G;
    return want < kSearchMaxLanes ? want : kSearchMaxLanes;
}

hipError_t launch_expectimax(const Boards &b, uint32_t depth, const SearchArgs &a, hipStream_t s)
{
    return dispatch<1, 3>(static_cast<int>(depth), [&](auto dc) {
        return dispatch_bool(b.plain, [&](auto plain_c) {
            return launch_1d(expectimax_kernel<dc, plain_c>, group_lanes(b.n, dc == 1 ? 4u : 64u), 0, s, b.ptr, b.n, a);
        });
    });
}

hipError_t launch_mc_search(const Boards &b, const McArgs &a, hipStream_t s)
{
    auto go = [&](auto gc) {
        return dispatch_bool(b.plain, [&](auto plain_c) {
            return launch_1d(mc_search_kernel<gc, plain_c>, group_lanes(b.n, gc), 0, s, b.ptr, b.n, a);
        });
    };
    return a.rollouts >= kMcWaveRollouts ? go(std::integral_constant<uint32_t, 64u>()) : go(std::integral_constant<uint32_t, 16u>());
}

// f(std::integral_constant<uint32_t, T>(), shape) for the network's tuple count T = 1..8 and its shape: an NtupleShape for
// one weight set -- the kernels of the unstaged network, whichever descriptor it came in -- an NtupleStagedShape for S > 1,
// and for a network with a cell list that ends early (G2048_NTUPLE_END), staged or not, an NtupleMixedShape
template <class F>
static hipError_t dispatch_tuples(const NtupleNet &net, F &&f)
{
    const bool mixed = ntuple_is_mixed(net.n_tuples, net.tuple_len, net.cells);
    const NtupleShape sh = ntuple_shape(net.n_tuples, net.tuple_len, net.cells);
    return dispatch<1, 8>(static_cast<int>(net.n_tuples), [&](auto tc) {
        const std::integral_constant<uint32_t, static_cast<uint32_t>(decltype(tc)::value)> t;
        if (mixed)
            return f(t, ntuple_mixed_shape(net.n_tuples, net.tuple_len, net.cells, net.n_stages, net.thresholds));
        return net.n_stages > 1 ? f(t, ntuple_staged_shape(sh, net.n_stages, net.thresholds)) : f(t, sh);
    });
}

hipError_t launch_ntuple_eval(const Boards &b, const NtupleNet &net, const NtupleOut &o, hipStream_t s)
{
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return dispatch_bool(b.plain, [&](auto plain_c) {
            return launch_1d(ntuple_eval_kernel<tc, plain_c, decltype(sh)>, group_lanes(b.n, 4u), 0, s, b.ptr, b.n, sh, net.frac_bits,
                             static_cast<const int32_t *>(net.weights), o);
        });
    });
}

hipError_t launch_ntuple_play(const StepArgs &a, const NtupleNet &net, const NtuplePlayOut &io, hipStream_t s)
{
    if (a.k_steps == 0)
        return hipSuccess;
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return launch_1d(ntuple_play_kernel<tc, decltype(sh)>, a.n, 0, s, a, sh, net.frac_bits, static_cast<const int32_t *>(net.weights), io);
    });
}

hipError_t launch_ntuple_play_downgraded(const StepArgs &a, const NtupleNet &net, const DowngradeArgs &rule, const NtuplePlayOut &io,
                                         hipStream_t s)
{
    if (a.k_steps == 0)
        return hipSuccess;
    const DowngradeRule r{rule.min_exp, rule.floor_exp};
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return launch_1d(ntuple_play_downgraded_kernel<tc, decltype(sh)>, a.n, 0, s, a, sh, net.frac_bits,
                         static_cast<const int32_t *>(net.weights), r, io);
    });
}

hipError_t launch_downgrade(const uint4 *boards, uint32_t n, const DowngradeArgs &rule, const uint32_t *active, uint4 *out,
                            uint8_t *missing, hipStream_t s)
{
    return launch_1d(downgrade_kernel, n, 0, s, boards, n, DowngradeRule{rule.min_exp, rule.floor_exp}, active, out, missing);
}

hipError_t launch_ntuple_td_step(const StepArgs &a, const NtupleNet &net, const NtupleTdIo &io, hipStream_t s)
{
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return launch_1d(ntuple_td_step_kernel<tc, decltype(sh)>, a.n, 0, s, a, sh, net.frac_bits, static_cast<const int32_t *>(net.weights), io);
    });
}

hipError_t launch_ntuple_play_log(const StepArgs &a, const NtupleNet &net, const NtupleLog &log, hipStream_t s)
{
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return launch_1d(ntuple_play_log_kernel<tc, decltype(sh)>, a.n, 0, s, a, sh, net.frac_bits, static_cast<const int32_t *>(net.weights),
                         log);
    });
}

static Restart restart_of(const RestartArgs &a)
{
    return Restart{RestartRule{a.stride_log2, a.capacity, a.min_span, a.max_restarts}, a.snap, a.pos, a.start, a.restarts};
}

hipError_t launch_ntuple_play_log_restart(const StepArgs &a, const NtupleNet &net, const NtupleLog &log, const RestartArgs &ra, hipStream_t s)
{
    const Restart rs = restart_of(ra);
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return launch_1d(ntuple_play_log_restart_kernel<tc, decltype(sh)>, a.n, 0, s, a, sh, net.frac_bits,
                         static_cast<const int32_t *>(net.weights), log, rs);
    });
}

hipError_t launch_restart_step(uint4 *records, const uint8_t *terminated, uint32_t n, const RestartArgs &ra, hipStream_t s)
{
    const Restart rs = restart_of(ra);
    const uint64_t groups = (static_cast<uint64_t>(n) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(restart_step_kernel, dim3(static_cast<uint32_t>(groups < kRestartMaxGroups ? groups : kRestartMaxGroups)), dim3(kBlock), 0,
                       s, records, terminated, n, rs);
    return hipGetLastError();
}

hipError_t launch_ntuple_log_delta(uint32_t n, const NtupleNet &net, const NtupleLog &log, uint32_t m, int64_t *delta, hipStream_t s)
{
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return launch_1d(ntuple_log_delta_kernel<tc, decltype(sh)>, n, 0, s, log, n, m, sh, static_cast<const int32_t *>(net.weights), delta);
    });
}

hipError_t launch_play_step(const StepArgs &a, int action_dtype, const NtuplePlayOut &io, hipStream_t s)
{
    return dispatch<0, 3>(action_dtype, [&](auto act) { return launch_1d(play_step_kernel<act>, a.n, 0, s, a, io); });
}

// f(std::bool_constant<PLAIN>(), std::bool_constant<MASKED>()) for the three forms the search kernels are built in: engine
// records under a mask, engine records, plain boards.  No <PLAIN, MASKED> form: the caller gives no mask for plain boards,
// and a fourth form would be 8 x 3 more kernels per search kernel and depth.
template <class F>
static hipError_t dispatch_search_form(const Boards &b, const uint32_t *active, F &&f)
{
    if (active)
        return f(std::false_type(), std::true_type());
    return dispatch_bool(b.plain, [&](auto plain_c) { return f(plain_c, std::false_type()); });
}

hipError_t launch_ntuple_search(const Boards &b, uint32_t depth, const NtupleNet &net, const NtupleSearchOut &o, hipStream_t s)
{
    return dispatch<1, static_cast<int>(kNtupleSearchMaxDepth)>(static_cast<int>(depth), [&](auto dc) {
        return dispatch_tuples(net, [&](auto tc, auto sh) {
            return dispatch_search_form(b, o.active, [&](auto plain_c, auto masked_c) {
                return launch_1d(ntuple_search_kernel<dc, tc, plain_c, decltype(sh), masked_c>, group_lanes(b.n, kNtupleSearchGroup<dc>), 0,
                                 s, b.ptr, b.n, sh, net.frac_bits, static_cast<const int32_t *>(net.weights), o);
            });
        });
    });
}

// One workgroup per board: group_lanes(n, kBlock) lanes, so at most kSearchMaxLanes / kBlock = 65 536 workgroups.
// -DG2048_PROBE_WAVE_DEPTH3 (never the product's build; `python tools/ntuple_deep_probe.py --build-wave-lib FILE` compiles such
// a library with build_hip's flags) sends depth 3 without a mask to the alternative this kernel was timed against:
// ntuple_search_kernel<3>, one wavefront per board.
hipError_t launch_ntuple_deep_search(const Boards &b, uint32_t depth, const NtupleNet &net, const NtupleSearchOut &o, hipStream_t s)
{
#ifdef G2048_PROBE_WAVE_DEPTH3
    if (depth == 3 && !o.active)
        return dispatch_tuples(net, [&](auto tc, auto sh) {
            return dispatch_bool(b.plain, [&](auto plain_c) {
                return launch_1d(ntuple_search_kernel<3, tc, plain_c, decltype(sh)>, group_lanes(b.n, kNtupleSearchGroup<3>), 0, s, b.ptr, b.n,
                                 sh, net.frac_bits, static_cast<const int32_t *>(net.weights), o);
            });
        });
#endif
    return dispatch<static_cast<int>(kNtupleDeepMinDepth), static_cast<int>(kNtupleDeepMaxDepth)>(static_cast<int>(depth), [&](auto dc) {
        return dispatch_tuples(net, [&](auto tc, auto sh) {
            return dispatch_search_form(b, o.active, [&](auto plain_c, auto masked_c) {
                return launch_1d(ntuple_deep_search_kernel<dc, tc, plain_c, decltype(sh), masked_c>, group_lanes(b.n, kBlock), 0, s, b.ptr,
                                 b.n, sh, net.frac_bits, static_cast<const int32_t *>(net.weights), o);
            });
        });
    });
}

// One workgroup per board, as launch_ntuple_deep_search; the depth is the kernel's own business
hipError_t launch_ntuple_adaptive_search(const Boards &b, const uint8_t schedule[17], const NtupleNet &net, const NtupleAdaptiveOut &o,
                                         hipStream_t s)
{
    const NtupleAdaptiveSchedule sc = ntuple_adaptive_schedule(schedule);
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return dispatch_search_form(b, o.active, [&](auto plain_c, auto masked_c) {
            return launch_1d(ntuple_adaptive_search_kernel<tc, plain_c, decltype(sh), masked_c>, group_lanes(b.n, kBlock), 0, s, b.ptr, b.n,
                             sh, net.frac_bits, static_cast<const int32_t *>(net.weights), sc, o);
        });
    });
}

// As launch_ntuple_adaptive_search; reduce4 in kNtupleReduce4Min..Max (checked by the caller) is the same for the whole launch
hipError_t launch_ntuple_reduced_search(const Boards &b, const uint8_t schedule[17], uint32_t reduce4, const NtupleNet &net,
                                        const NtupleAdaptiveOut &o, hipStream_t s)
{
    const NtupleAdaptiveSchedule sc = ntuple_adaptive_schedule(schedule);
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return dispatch_search_form(b, o.active, [&](auto plain_c, auto masked_c) {
            return launch_1d(ntuple_reduced_search_kernel<tc, plain_c, decltype(sh), masked_c>, group_lanes(b.n, kBlock), 0, s, b.ptr, b.n,
                             sh, net.frac_bits, static_cast<const int32_t *>(net.weights), sc, reduce4, o);
        });
    });
}

hipError_t launch_ntuple_values(const uint4 *boards, uint32_t n, const NtupleNet &net, int64_t *v, hipStream_t s)
{
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return launch_1d(ntuple_values_kernel<tc, decltype(sh)>, n, 0, s, boards, n, sh, static_cast<const int32_t *>(net.weights), v);
    });
}

hipError_t launch_ntuple_stage(const uint4 *boards, uint32_t n, const NtupleNet &net, uint8_t *stage, hipStream_t s)
{
    const NtupleStagedShape sh = ntuple_staged_shape(ntuple_shape(net.n_tuples, net.tuple_len, net.cells), net.n_stages, net.thresholds);
    return launch_1d(ntuple_stage_kernel, n, 0, s, boards, n, sh, stage);
}

// One lane per item of the source, up to the grid cap
template <class Items> static uint64_t item_lanes(const Items &items)
{
    return items.size() < kSearchMaxLanes ? items.size() : kSearchMaxLanes;
}

template <class Items>
static hipError_t launch_items_update(const Items &items, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net, hipStream_t s)
{
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        return launch_1d(ntuple_update_kernel<tc, decltype(sh), Items>, item_lanes(items), 0, s, items, delta, lr_shift, sh, net.weights);
    });
}

// phase W, then phase A, a launch each
template <class Items>
static hipError_t launch_items_tc_update(const Items &items, const int64_t *delta, uint32_t lr_shift, uint32_t phases, const NtupleNet &net,
                                         int64_t *err, int64_t *mag, hipStream_t s)
{
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        if (phases & kNtupleTcWeights) {
            const hipError_t rc = launch_1d(ntuple_tc_weights_kernel<tc, decltype(sh), Items>, item_lanes(items), 0, s, items, delta, lr_shift,
                                            sh, net.weights, static_cast<const int64_t *>(err), static_cast<const int64_t *>(mag));
            if (rc != hipSuccess)
                return rc;
        }
        if (phases & kNtupleTcAccum)
            return launch_1d(ntuple_tc_accum_kernel<tc, decltype(sh), Items>, item_lanes(items), 0, s, items, delta, sh, err, mag);
        return hipSuccess;
    });
}

// phase SUM, then phase APPLY, a launch each
template <class Items>
static hipError_t launch_items_mean_update(const Items &items, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                           const NtupleMean &mean, hipStream_t s)
{
    return dispatch_tuples(net, [&](auto tc, auto sh) {
        if (mean.phases & kNtupleMeanSum) {
            const hipError_t rc =
                launch_1d(ntuple_mean_sum_kernel<tc, decltype(sh), Items>, item_lanes(items), 0, s, items, delta, sh, mean.sum, mean.count);
            if (rc != hipSuccess)
                return rc;
        }
        if (mean.phases & kNtupleMeanApply)
            return launch_1d(ntuple_mean_apply_kernel<tc, decltype(sh), Items>, item_lanes(items), 0, s, items, delta, lr_shift, sh,
                             net.weights, mean.sum, mean.count);
        return hipSuccess;
    });
}

hipError_t launch_ntuple_mean_update(const uint4 *boards, uint32_t n, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                     const NtupleMean &mean, hipStream_t s)
{
    return launch_items_mean_update(NtupleBoardItems{boards, n}, delta, lr_shift, net, mean, s);
}

hipError_t launch_ntuple_mean_trace_update(uint32_t n, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                           const NtupleTrace &tr, uint32_t slot, const NtupleMean &mean, hipStream_t s)
{
    return launch_items_mean_update(NtupleTraceItems{tr.hist, tr.len, n, tr.depth, tr.lambda, slot}, delta, lr_shift, net, mean, s);
}

// The three updates: the TD update of the item source, or with accumulators its TC update
hipError_t launch_ntuple_update(const uint4 *boards, uint32_t n, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                const NtupleTc *tc, hipStream_t s)
{
    const NtupleBoardItems items{boards, n};
    if (!tc)
        return launch_items_update(items, delta, lr_shift, net, s);
    return launch_items_tc_update(items, delta, lr_shift, tc->phases, net, tc->err, tc->mag, s);
}

hipError_t launch_ntuple_push(const uint4 *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated,
                              uint32_t n, const NtupleTrace &tr, uint32_t slot, int64_t *delta, hipStream_t s)
{
    return launch_1d(ntuple_trace_push_kernel, group_lanes(n, 1u), 0, s, after, after_value, best_next, terminated, n, tr.depth,
                     tr.hist + static_cast<uint64_t>(slot) * n, tr.len, delta);
}

hipError_t launch_ntuple_trace_update(uint32_t n, const int64_t *delta, uint32_t lr_shift, const NtupleNet &net,
                                      const NtupleTrace &tr, uint32_t slot, const NtupleTc *tc, hipStream_t s)
{
    const NtupleTraceItems items{tr.hist, tr.len, n, tr.depth, tr.lambda, slot};
    if (!tc)
        return launch_items_update(items, delta, lr_shift, net, s);
    return launch_items_tc_update(items, delta, lr_shift, tc->phases, net, tc->err, tc->mag, s);
}

hipError_t launch_ntuple_push(const uint4 *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated,
                              uint32_t n, const NtupleDelay &dl, uint32_t slot, int64_t *delta, hipStream_t s)
{
    return launch_1d(ntuple_delay_push_kernel, group_lanes(n, 1u), 0, s, after, after_value, best_next, terminated, n, dl.depth,
                     dl.lambda, slot, dl.hist + static_cast<uint64_t>(slot) * n, dl.len, dl.acc, delta);
}

// the accumulators go where the other sources' delta goes (NtupleDelayItems, g2048_device.h)
hipError_t launch_ntuple_delay_update(uint32_t n, uint32_t lr_shift, uint32_t mode, const NtupleNet &net, const NtupleDelay &dl,
                                      uint32_t slot, const NtupleTc *tc, hipStream_t s)
{
    const NtupleDelayItems items{dl.hist, dl.len, n, dl.depth, slot, mode};
    if (!tc)
        return launch_items_update(items, dl.acc, lr_shift, net, s);
    return launch_items_tc_update(items, dl.acc, lr_shift, tc->phases, net, tc->err, tc->mag, s);
}

hipError_t launch_carousel_step(const CarouselArgs &a, hipStream_t s)
{
    CarouselParams p{a.records, a.terminated, a.pool, a.count, a.seen, a.episodes, a.scratch, carousel_stages(a.n_stages, a.thresholds),
                     a.n,       a.index_offset, a.n_stages, a.capacity, a.seed_lo, a.seed_hi, carousel_range(a.n, kBlock, kCarouselMaxGroups)};
    const uint32_t groups = static_cast<uint32_t>((a.n + p.per - 1u) / p.per); // <= kCarouselMaxGroups
    hipLaunchKernelGGL(carousel_restart_kernel, dim3(groups), dim3(kBlock), 0, s, p);
    if (const hipError_t rc = hipGetLastError(); rc != hipSuccess)
        return rc;
    hipLaunchKernelGGL(carousel_scan_kernel, dim3(1), dim3(kBlock), 0, s, p, groups);
    if (const hipError_t rc = hipGetLastError(); rc != hipSuccess)
        return rc;
    hipLaunchKernelGGL(carousel_scatter_kernel, dim3(groups), dim3(kBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_add_tile(const StepArgs &a, uint32_t slot, hipStream_t s)
{
    if (a.st.rng)
        return launch_1d(add_tile_numpy_kernel, a.n, 0, s, a);
    return launch_1d(add_tile_kernel, a.n, 0, s, a, slot);
}

hipError_t launch_seed_numpy(uint64_t *planes, uint32_t n, uint64_t first_seed, hipStream_t s)
{
    return launch_1d(seed_numpy_kernel, n, 0, s, planes, n, first_seed);
}

// ---- a k-step launch train as a CACHED hipGraph (small batches)
// At 65 536 boards a step kernel takes ~2.4 us on the device and one host thread issues a launch every 3.0-4.6 us: the
// per-step path is host-issue-bound (tools/ubench/r5_probe.hip: 3.0-4.6 us per step by stream launches, 2.43-2.45 us as a
// graph replay; 2^17 boards 2.9-3.6 vs 2.95-2.99; from 2^18 boards on the kernel is the longer of the two and the forms tie).
// The graph is k x step_graph_kernel, explicit nodes in a chain; building and instantiating it costs ~1.8 us per node (less
// than launching the same train once), replaying it one set_clock_kernel launch (the new clock value) + one hipGraphLaunch.
bool rollout_graph_supported(const StepArgs &a)
{
    return a.n != 0 && standard_outputs(a) && !a.obs && !a.st.rng && !a.action_err;
}

void destroy_rollout_graph(RolloutGraph &g)
{
    if (g.exec)
        (void)hipGraphExecDestroy(g.exec);
    if (g.graph)
        (void)hipGraphDestroy(g.graph);
    g.exec = nullptr;
    g.graph = nullptr;
}

// `first`: the arguments of step 0 (its t is ignored); step j reads / writes its I/O j * stride elements further on.
hipError_t build_rollout_graph(const StepArgs &first, int action_dtype, uint32_t k_steps, uint64_t stride, unsigned long long *t_dev,
                               RolloutGraph *out)
{
    static const size_t act_bytes[4] = {0, 1, 4, 8};
    void *fn = nullptr;
    const hipError_t known = dispatch_step(action_dtype, first.n % kBlock == 0, [&](auto act, auto full) {
        fn = reinterpret_cast<void *>(step_graph_kernel<act, full>);
        return hipSuccess;
    });
    if (known != hipSuccess || !rollout_graph_supported(first) || !t_dev || !out)
        return hipErrorInvalidValue;
    RolloutGraph g{};
    g.t_dev = t_dev;
    hipError_t err = hipGraphCreate(&g.graph, 0);
    if (err != hipSuccess)
        return err;
    hipGraphNode_t prev = nullptr;
    for (uint32_t j = 0; j < k_steps && err == hipSuccess; ++j) {
        const size_t off = static_cast<size_t>(j) * stride;
        uint4 *boards = first.st.boards;
        const void *actions = first.actions ? static_cast<const char *>(first.actions) + off * act_bytes[action_dtype] : nullptr;
        unsigned long long *ep = first.st.ep_counters;
        uint32_t board_offset = first.board_offset, seed_lo = first.seed_lo, seed_hi = first.seed_hi, n = first.n, jj = j;
        const unsigned long long *t_ptr = t_dev;
        float *reward = first.reward + off;
        StepTail tail = step_tail(first); // (the standard configuration: its optional outputs are NULL)
        tail.terminated += off;
        tail.obs_dtype = 0u;
        tail.done_value = 0ull;
        void *args[11] = {&boards, &actions, &ep, &board_offset, &seed_lo, &seed_hi, &t_ptr, &n, &jj, &reward, &tail};
        hipKernelNodeParams kp{};
        kp.func = fn;
        kp.gridDim = grid_for(first.n);
        kp.blockDim = dim3(kBlock);
        kp.kernelParams = args;
        hipGraphNode_t node = nullptr;
        err = hipGraphAddKernelNode(&node, g.graph, prev ? &prev : nullptr, prev ? 1 : 0, &kp);
        prev = node;
    }
    if (err == hipSuccess)
        err = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
    if (err != hipSuccess) {
        destroy_rollout_graph(g);
        return err;
    }
    *out = g;
    return hipSuccess;
}

// Replay: step j of the train plays transaction t_first + j.  The clock is written by an ORDINARY launch in front of the
// graph -- its value is captured when it is enqueued, so two replays enqueued back to back each see their own (an executable
// graph's node parameters must not be rewritten while an earlier launch of it may still be waiting to run).
hipError_t launch_rollout_graph(RolloutGraph &g, unsigned long long t_first, hipStream_t s)
{
    hipLaunchKernelGGL(set_clock_kernel, dim3(1), dim3(64), 0, s, g.t_dev, t_first);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return err;
    return hipGraphLaunch(g.exec, s);
}

hipError_t launch_rollout_fused(const StepArgs &a, int action_dtype, uint64_t stride, hipStream_t s)
{
    if (a.n == 0 || a.k_steps == 0)
        return hipSuccess;
    return dispatch<0, 3>(action_dtype, [&](auto act) {
        if (a.st.rng) // numpy-RNG mode: the lanes of a wavefront drift in time (rollout_fused_numpy_kernel)
            return launch_1d(rollout_fused_numpy_kernel<act>, a.n, 0, s, a, stride);
        return launch_1d(rollout_fused_kernel<act>, a.n, 0, s, a, stride);
    });
}

hipError_t launch_rollout_random(const StepArgs &a, hipStream_t s)
{
    if (a.st.rng) // numpy-RNG mode: the fused form of that mode with the synthetic policy and no per-step output
        return launch_rollout_fused(a, 0, 0, s);
    return a.k_steps == 0 ? hipSuccess : launch_1d(rollout_random_kernel, a.n, 0, s, a);
}

hipError_t launch_fill_actions(uint8_t *out, uint32_t n, uint32_t board_offset, uint32_t seed_lo, uint32_t seed_hi,
                               uint64_t t_first, uint32_t k_steps, hipStream_t s)
{
    if (n == 0 || k_steps == 0)
        return hipSuccess;
    // gridDim.y is limited to 65535: walk the step axis in slabs.
    for (uint32_t j0 = 0; j0 < k_steps; j0 += 32768u) {
        const uint32_t kj = (k_steps - j0 < 32768u) ? (k_steps - j0) : 32768u;
        dim3 g(grid_for(n).x, kj);
        hipLaunchKernelGGL(fill_actions_kernel, g, dim3(kBlock), 0, s, out + static_cast<size_t>(j0) * n, n,
                           board_offset, seed_lo, seed_hi, t_first + j0, kj);
    }
    return hipGetLastError();
}

hipError_t launch_onehot(const uint4 *boards, uint32_t n, void *out, int obs_dtype, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    return dispatch<0, 2>(obs_dtype, [&](auto obs) {
        const uint64_t chunks = static_cast<uint64_t>(n) * (16u << obs); // 16-byte chunks: 16 / 32 / 64 per board
        return launch_1d(onehot_kernel<obs>, chunks, 0, s, boards, chunks, static_cast<uint4 *>(out));
    });
}

hipError_t launch_augment(const uint4 *boards, const uint4 *next_boards, const uint8_t *actions, uint32_t n,
                          uint4 *boards_out, uint4 *next_out, uint8_t *actions_out, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(augment_kernel, dim3(grid_for(n).x, 8), dim3(kBlock), 0, s, boards, next_boards, actions, n,
                       boards_out, next_out, actions_out);
    return hipGetLastError();
}

hipError_t launch_stats(const DeviceState &st, uint32_t n, unsigned long long *partials, unsigned long long *summary_scratch,
                        StatsOut *dev_out, bool returns_only, hipStream_t s)
{
    uint32_t blocks = grid_for(n).x;
    if (blocks > kStatsBlocks)
        blocks = kStatsBlocks;
    if (blocks == 0)
        blocks = 1; // n == 0: one block writes an all-zero partial
    if (returns_only) {
        // ONE launch: at most kSummaryBlocks blocks of sixteen wavefronts, merged by "last one out" (see the kernel)
        const uint32_t n_waves = (n + 63u) / 64u;
        uint32_t sblocks = (n_waves + kSummaryThreads / 64u - 1u) / (kSummaryThreads / 64u);
        sblocks = sblocks == 0u ? 1u : (sblocks > kSummaryBlocks ? kSummaryBlocks : sblocks);
        hipLaunchKernelGGL(returns_summary_kernel, dim3(sblocks), dim3(kSummaryThreads), 0, s, st, n, n_waves, summary_scratch, dev_out);
    } else {
        hipLaunchKernelGGL(stats_kernel, dim3(blocks), dim3(kBlock), 0, s, st, n, (n + 63u) / 64u, partials);
        hipLaunchKernelGGL(stats_merge_kernel, dim3(kStatsFields), dim3(kBlock), 0, s, partials, blocks, dev_out,
                           st.last_record != nullptr);
    }
    return hipGetLastError();
}

hipError_t launch_export_boards(const uint4 *records, uint32_t n, uint4 *cells_out, hipStream_t s)
{
    return launch_1d(export_boards_kernel, n, 0, s, records, n, cells_out);
}

hipError_t launch_import_boards(uint4 *records, uint32_t n, const uint4 *cells_in, hipStream_t s)
{
    return launch_1d(import_boards_kernel, n, 0, s, records, n, cells_in);
}

hipError_t launch_export_scores(const uint4 *records, uint32_t n, int32_t *scores_out, hipStream_t s)
{
    return launch_1d(export_scores_kernel, n, 0, s, records, n, scores_out);
}

hipError_t launch_import_scores(uint4 *records, uint32_t n, const int32_t *scores_in, unsigned long long *ep_counters,
                                hipStream_t s)
{
    return launch_1d(import_scores_kernel, n, 0, s, records, n, scores_in, ep_counters);
}

hipError_t launch_clear_stats(const DeviceState &st, uint32_t n, hipStream_t s)
{
    return launch_1d(clear_stats_kernel, n, 0, s, st, n);
}

hipError_t launch_export_last_scores(const DeviceState &st, uint32_t n, int32_t *out, hipStream_t s)
{
    return launch_1d(export_last_scores_kernel, n, 0, s, st.last_record, n, out);
}

// get_board + self.score of every board in one launch, for the host-resident path
__global__ void __launch_bounds__(kBlock) fetch_kernel(const uint4 *records, uint32_t n, uint4 *cells_out, int32_t *scores_out,
                                                       unsigned long long *done_seq, unsigned long long done_value)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const Board raw = load_board(records, i);
        store_board(cells_out, i, record_cells(raw));
        scores_out[i] = static_cast<int32_t>(record_score(raw));
    }
    if (done_seq)
        signal_done(done_seq, done_value);
}

hipError_t launch_fetch(const uint4 *records, uint32_t n, uint4 *cells_out, int32_t *scores_out, unsigned long long *done_seq,
                        unsigned long long done_value, hipStream_t s)
{
    const dim3 g = grid_for(n);
    hipLaunchKernelGGL(fetch_kernel, g, dim3(kBlock), 0, s, records, n, cells_out, scores_out, done_seq, done_value);
    if (done_seq && g.x > 1)
        hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(64), 0, s, done_seq, done_value);
    return hipGetLastError();
}

hipError_t launch_flag_set(unsigned long long *flag, unsigned long long value, hipStream_t s)
{
    hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(64), 0, s, flag, value);
    return hipGetLastError();
}

hipError_t launch_flag_wait(const unsigned long long *flag, unsigned long long value, unsigned long long *timed_out,
                            uint32_t max_polls, hipStream_t s)
{
    hipLaunchKernelGGL(flag_wait_kernel, dim3(1), dim3(64), 0, s, flag, value, timed_out, max_polls);
    return hipGetLastError();
}

hipError_t launch_signal(unsigned long long *done_seq, unsigned long long done_value, hipStream_t s)
{
    hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(64), 0, s, done_seq, done_value);
    return hipGetLastError();
}

hipError_t launch_canonicalize(uint4 *boards, uint4 *next_boards, uint8_t *actions, uint32_t n, uint8_t *sym_out,
                               hipStream_t s)
{
    return launch_1d(canonicalize_kernel, n, 0, s, boards, next_boards, actions, n, sym_out);
}

} // namespace g2048
