// ntuple_staged_check.cpp -- the multi-stage n-tuple code of g2048_device.h (the header the kernels are compiled from) built
// for the host (-DG2048_HOST_CHECK), one board at a time on one thread: the mask, the stage, and every per-board function
// with an NtupleStagedShape (S = 1 included: the staged code with no threshold).  tests/test_ntuple_staged_host.py compares it with the pure-Python reference
// (tests/ntuple_staged_ref.py); the GPU tests compare the kernels with that reference too.  Not part of the product.
#define G2048_HOST_CHECK 1
#include "../../gym-2048_amd/csrc/g2048_device.h"

#include <cstring>
#include <type_traits>

using namespace g2048;

namespace {

const uint32_t kLut[32] = {G2048_MOVE_LUT_WORDS};

struct HostTables { // what LdsTables is on the device (g2048_kernels.hip)
    MoveSel move_sel(uint32_t action) const
    {
        const uint32_t *r = kLut + 8 * (action & 3u);
        return MoveSel{r[0], r[1], r[2], r[3], r[4], r[5]};
    }
};

// plain cells, taken mod 32 as input_cells<true> takes them on the device
Board load_cells(const uint8_t *p)
{
    Board b;
    memcpy(b.r, p, 16);
    for (uint32_t &r : b.r)
        r &= 0x1f1f1f1fu;
    return b;
}

// the 16 bytes as they are: what ntuple_pack sees of an engine record (score-deficit bits in bits 5..7 of bytes 8..15)
Board load_raw(const uint8_t *p)
{
    Board b;
    memcpy(b.r, p, 16);
    return b;
}

// the network a test describes (ctypes: ntuple_staged_helpers.Desc)
struct Desc {
    uint32_t T, L, F, S;
    uint16_t thr[8]; // the first S - 1 used
    uint8_t cells[8][6];
};

bool desc_ok(const Desc *d)
{
    return d && d->T >= 1 && d->T <= kNtupleMaxTuples && d->L >= 1 && d->L <= kNtupleMaxLen && d->F <= kNtupleMaxFrac && d->S >= 1 &&
           d->S <= kNtupleMaxStages;
}

NtupleStagedShape shape_of(const Desc *d) { return ntuple_staged_shape(ntuple_shape(d->T, d->L, d->cells), d->S, d->thr); }

// f(std::integral_constant<uint32_t, T>()) for the run-time T in 1..8
template <uint32_t T = 1, class F> void with_tuples(uint32_t n_tuples, F &&f)
{
    if constexpr (T <= kNtupleMaxTuples) {
        if (n_tuples == T)
            f(std::integral_constant<uint32_t, T>());
        else
            with_tuples<T + 1>(n_tuples, f);
    }
}

// f(d_k, packed afterstate) for every work item of a trace update, in the kernel's item order
template <class F>
void for_items(uint64_t n, const int64_t *delta, uint32_t H, uint32_t lam, const uint8_t *hist, const uint8_t *len, uint32_t slot, F f)
{
    for (uint64_t item = 0; item < H * n; ++item) {
        uint32_t k, i;
        ntuple_trace_split(item, static_cast<uint32_t>(n), H, k, i);
        const int64_t dk = ntuple_trace_item(len[i], delta[i], k, H, lam);
        if (dk != 0)
            f(dk, ntuple_pack(load_cells(hist + (static_cast<uint64_t>(ntuple_trace_slot(slot, k, H)) * n + i) * 16)));
    }
}

} // namespace

extern "C" {

// mask of n boards given as raw bytes: out[i] = ntuple_stage_mask(ntuple_pack(bytes))
void ntuple_staged_check_mask(const uint8_t *boards, uint64_t n, uint32_t *out)
{
    for (uint64_t i = 0; i < n; ++i)
        out[i] = ntuple_stage_mask(ntuple_pack(load_raw(boards + 16 * i)));
}

// stage of n boards given as raw bytes; -1 for a description out of range
int ntuple_staged_check_stage(const uint8_t *boards, uint64_t n, const Desc *d, uint8_t *out)
{
    if (!desc_ok(d))
        return -1;
    const NtupleStagedShape sh = shape_of(d);
    for (uint64_t i = 0; i < n; ++i)
        out[i] = static_cast<uint8_t>(ntuple_stage(ntuple_stage_mask(ntuple_pack(load_raw(boards + 16 * i))), sh));
    return 0;
}

// element offset of the weight set of n plain boards (ntuple_stage_base): what the look-ups add
int ntuple_staged_check_base(const uint8_t *boards, uint64_t n, const Desc *d, uint32_t *out)
{
    if (!desc_ok(d))
        return -1;
    const NtupleStagedShape sh = shape_of(d);
    for (uint64_t i = 0; i < n; ++i)
        out[i] = ntuple_stage_base(ntuple_pack(load_cells(boards + 16 * i)), sh);
    return 0;
}

int ntuple_staged_check_evaluate(const uint8_t *boards, uint64_t n, const Desc *d, const int32_t *weights, int64_t *value,
                                 uint8_t *action, int64_t *best, uint8_t *after, int64_t *after_value)
{
    if (!desc_ok(d))
        return -1;
    const NtupleStagedShape sh = shape_of(d);
    with_tuples(d->T, [&](auto tc) {
        for (uint64_t i = 0; i < n; ++i) {
            const NtupleRoot r = ntuple_root<decltype(tc)::value>(load_cells(boards + 16 * i), sh, d->F, weights, HostTables());
            memcpy(value + 4 * i, r.q, sizeof(r.q));
            action[i] = static_cast<uint8_t>(r.action);
            best[i] = r.best;
            memcpy(after + 16 * i, r.after.r, 16);
            after_value[i] = r.after_value;
        }
    });
    return 0;
}

int ntuple_staged_check_values(const uint8_t *boards, uint64_t n, const Desc *d, const int32_t *weights, int64_t *v)
{
    if (!desc_ok(d))
        return -1;
    const NtupleStagedShape sh = shape_of(d);
    with_tuples(d->T, [&](auto tc) {
        for (uint64_t i = 0; i < n; ++i)
            v[i] = ntuple_value<decltype(tc)::value>(ntuple_pack(load_cells(boards + 16 * i)), sh, weights);
    });
    return 0;
}

// ntuple_search_root of n plain boards: action[n], value[n][4]
int ntuple_staged_check_search(const uint8_t *boards, uint64_t n, uint32_t depth, const Desc *d, const int32_t *weights,
                               uint8_t *action, int64_t *value)
{
    if (!desc_ok(d) || depth < 1 || depth > kNtupleSearchMaxDepth)
        return -1;
    const NtupleStagedShape sh = shape_of(d);
    with_tuples(d->T, [&](auto tc) {
        constexpr uint32_t TT = decltype(tc)::value;
        for (uint64_t i = 0; i < n; ++i) {
            const Board b = load_cells(boards + 16 * i);
            action[i] = static_cast<uint8_t>(depth == 1 ? ntuple_search_root<1, TT>(b, sh, d->F, weights, HostTables(), value + 4 * i)
                                                        : ntuple_search_root<2, TT>(b, sh, d->F, weights, HostTables(), value + 4 * i));
        }
    });
    return 0;
}

// One-step updates of n plain boards, in place on weights / err / mag ([S][T][16^L]).  mode 0: the TD(0) update; mode 1..3:
// the TC update with phases = mode, phase W over every board, then phase A over every board.
int ntuple_staged_check_update(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t mode, const Desc *d,
                               int32_t *weights, int64_t *err, int64_t *mag)
{
    if (!desc_ok(d) || lr_shift > kNtupleMaxShift || mode > 3)
        return -1;
    const NtupleStagedShape sh = shape_of(d);
    uint32_t *w = reinterpret_cast<uint32_t *>(weights);
    uint64_t *e = reinterpret_cast<uint64_t *>(err), *a = reinterpret_cast<uint64_t *>(mag);
    with_tuples(d->T, [&](auto tc) {
        constexpr uint32_t TT = decltype(tc)::value;
        auto add32 = [w](uint32_t off, int32_t st) { w[off] += static_cast<uint32_t>(st); };
        auto for_boards = [&](auto f) {
            for (uint64_t i = 0; i < n; ++i)
                f(delta[i], ntuple_pack(load_cells(boards + 16 * i)));
        };
        if (mode == 0)
            for_boards([&](int64_t dl, uint64_t packed) {
                const int32_t step = ntuple_step(dl, lr_shift);
                if (step != 0)
                    ntuple_update<TT>(packed, sh, step, add32);
            });
        if (mode & 1u)
            for_boards([&](int64_t dl, uint64_t packed) {
                if (const int64_t dd = ntuple_tc_delta(dl))
                    ntuple_tc_weights<TT>(packed, sh, dd, lr_shift, err, mag, add32);
            });
        if (mode & 2u)
            for_boards([&](int64_t dl, uint64_t packed) {
                if (const int64_t dd = ntuple_tc_delta(dl))
                    ntuple_tc_accum<TT>(packed, sh, dd, [e, a](uint32_t off, int64_t x, uint64_t m) {
                        e[off] += static_cast<uint64_t>(x);
                        a[off] += m;
                    });
            });
    });
    return 0;
}

// The trace update of n boards, in place; mode as above.
int ntuple_staged_check_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t mode, const Desc *d, int32_t *weights,
                                     int64_t *err, int64_t *mag, uint32_t H, uint32_t lam, const uint8_t *hist, const uint8_t *len,
                                     uint32_t slot)
{
    if (!desc_ok(d) || lr_shift > kNtupleMaxShift || mode > 3 || H < 1 || H > kNtupleTraceMax || lam > kNtupleTcOne || slot >= H)
        return -1;
    const NtupleStagedShape sh = shape_of(d);
    uint32_t *w = reinterpret_cast<uint32_t *>(weights);
    uint64_t *e = reinterpret_cast<uint64_t *>(err), *a = reinterpret_cast<uint64_t *>(mag);
    with_tuples(d->T, [&](auto tc) {
        constexpr uint32_t TT = decltype(tc)::value;
        auto add32 = [w](uint32_t off, int32_t st) { w[off] += static_cast<uint32_t>(st); };
        if (mode == 0)
            for_items(n, delta, H, lam, hist, len, slot, [&](int64_t dk, uint64_t packed) {
                const int32_t step = ntuple_step(dk, lr_shift);
                if (step != 0)
                    ntuple_update<TT>(packed, sh, step, add32);
            });
        if (mode & 1u)
            for_items(n, delta, H, lam, hist, len, slot,
                      [&](int64_t dk, uint64_t packed) { ntuple_tc_weights<TT>(packed, sh, dk, lr_shift, err, mag, add32); });
        if (mode & 2u)
            for_items(n, delta, H, lam, hist, len, slot, [&](int64_t dk, uint64_t packed) {
                ntuple_tc_accum<TT>(packed, sh, dk, [e, a](uint32_t off, int64_t x, uint64_t m) {
                    e[off] += static_cast<uint64_t>(x);
                    a[off] += m;
                });
            });
    });
    return 0;
}

} // extern "C"
