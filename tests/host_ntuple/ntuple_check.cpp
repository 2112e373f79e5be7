// ntuple_check.cpp -- the n-tuple code of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK) on one thread: the network, its expectimax, the TD, TC and trace updates and the stages.  The
// updates run the header's item sources, item loop and per-item operations -- what the update kernels run -- with
// wrapping adds for the atomic ones.  tests/test_ntuple*_host.py compare it with the pure-Python references
// (tests/ntuple*_ref.py); the GPU tests compare the kernels with those references too.  Not part of the product.
#include "../host_common/ntuple_host.h"

namespace {

constexpr uint32_t kMaxKind = 1; // the calls instantiate NtupleShape (S == 1) and NtupleStagedShape, S = 1 included

NtupleStagedShape staged_shape_of(const Desc *d) { return ntuple_staged_shape(ntuple_shape(d->T, d->L, d->cells), d->S, d->thr); }

// The update of every item of a source, in place on weights / err / mag.  mode 0: the TD update; mode 1..3: the TC update
// with phases = mode, phase W over every item, then phase A over every item.
template <class Items>
int update_items(const Items &items, const int64_t *delta, uint32_t lr_shift, uint32_t mode, const Desc *d, int32_t *weights, int64_t *err,
                 int64_t *mag)
{
    if (!desc_ok(d, kMaxKind) || lr_shift > kNtupleMaxShift || mode > 3)
        return -1;
    uint32_t *w = reinterpret_cast<uint32_t *>(weights);
    uint64_t *e = reinterpret_cast<uint64_t *>(err), *a = reinterpret_cast<uint64_t *>(mag);
    auto add = [w](uint32_t off, int32_t step) { w[off] += static_cast<uint32_t>(step); };
    auto accum = [e, a](uint32_t off, int64_t dd, uint64_t m) {
        e[off] += static_cast<uint64_t>(dd);
        a[off] += m;
    };
    using Item = typename Items::Item;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        if (mode == 0)
            ntuple_for_items(items, 0, 1, [&](Item it) { ntuple_item_update<T>(items, delta, it, lr_shift, sh, add); });
        if (mode & 1u)
            ntuple_for_items(items, 0, 1, [&](Item it) { ntuple_item_tc_weights<T>(items, delta, it, lr_shift, sh, err, mag, add); });
        if (mode & 2u)
            ntuple_for_items(items, 0, 1, [&](Item it) { ntuple_item_tc_accum<T>(items, delta, it, sh, accum); });
    });
    return 0;
}

const uint4 *as_boards(const uint8_t *p) { return reinterpret_cast<const uint4 *>(p); }

} // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------ scalar probes
int32_t ntuple_check_step(int64_t delta, uint32_t lr_shift) { return ntuple_step(delta, lr_shift); }

// the eight cell maps, out[8][16]: out[s][c] = ntuple_sym_cell(s, c)
void ntuple_check_sym_cells(uint8_t *out)
{
    for (uint32_t s = 0; s < 8; ++s)
        for (uint32_t c = 0; c < 16; ++c)
            out[16 * s + c] = static_cast<uint8_t>(ntuple_sym_cell(s, c));
}

int64_t ntuple_check_floor_div(int64_t a, int64_t b) { return floor_div(a, b); }

uint32_t ntuple_check_tc_rate(int64_t err, uint64_t mag) { return ntuple_tc_rate(err, mag); }

// step of an unclamped delta: the clamp is part of what is checked
int32_t ntuple_check_tc_step(int64_t delta, uint32_t rate, uint32_t lr_shift)
{
    return ntuple_tc_step(ntuple_tc_delta(delta), rate, lr_shift);
}

uint32_t ntuple_check_decay(uint32_t lam, uint32_t k) { return ntuple_trace_decay(lam, k); }

// d_k of an unclamped delta: the clamp is part of what is checked
int64_t ntuple_check_dk(int64_t delta, uint32_t lam, uint32_t k)
{
    return ntuple_trace_dk(ntuple_tc_delta(delta), ntuple_trace_decay(lam, k));
}

uint32_t ntuple_check_push_len(uint32_t old, uint32_t H, uint32_t terminated) { return ntuple_trace_push_len(old, H, terminated != 0); }

uint32_t ntuple_check_len(uint32_t len, uint32_t H) { return ntuple_trace_len(len, H); }

// (k << 32) | i of a work item
uint64_t ntuple_check_split(uint64_t item, uint32_t n, uint32_t H)
{
    uint32_t k, i;
    ntuple_trace_split(item, n, H, k, i);
    return static_cast<uint64_t>(k) << 32 | i;
}

// mask of n boards given as raw bytes: out[i] = ntuple_stage_mask(ntuple_pack(bytes))
void ntuple_check_mask(const uint8_t *boards, uint64_t n, uint32_t *out)
{
    for (uint64_t i = 0; i < n; ++i)
        out[i] = ntuple_stage_mask(ntuple_pack(load_raw(boards + 16 * i)));
}

// stage of n boards given as raw bytes; -1 for a description out of range
int ntuple_check_stage(const uint8_t *boards, uint64_t n, const Desc *d, uint8_t *out)
{
    if (!desc_ok(d, kMaxKind))
        return -1;
    const NtupleStagedShape sh = staged_shape_of(d);
    for (uint64_t i = 0; i < n; ++i)
        out[i] = static_cast<uint8_t>(ntuple_stage(ntuple_stage_mask(ntuple_pack(load_raw(boards + 16 * i))), sh));
    return 0;
}

// element offset of the weight set of n plain boards (ntuple_stage_base): what the look-ups add
int ntuple_check_base(const uint8_t *boards, uint64_t n, const Desc *d, uint32_t *out)
{
    if (!desc_ok(d, kMaxKind))
        return -1;
    with_tuples(d, [&](auto, const auto &sh) {
        for (uint64_t i = 0; i < n; ++i)
            out[i] = ntuple_stage_base(ntuple_pack(load_cells(boards + 16 * i)), sh);
    });
    return 0;
}

// ------------------------------------------------------------------------------------------------ evaluate, values, search
// evaluate of n plain boards: value[n][4], action[n], best[n], after[n][16], after_value[n]; -1 for a description out of range
int ntuple_check_evaluate(const uint8_t *boards, uint64_t n, const Desc *d, const int32_t *weights, int64_t *value, uint8_t *action,
                          int64_t *best, uint8_t *after, int64_t *after_value)
{
    if (!desc_ok(d, kMaxKind))
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
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

int ntuple_check_values(const uint8_t *boards, uint64_t n, const Desc *d, const int32_t *weights, int64_t *v)
{
    if (!desc_ok(d, kMaxKind))
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
        for (uint64_t i = 0; i < n; ++i)
            v[i] = ntuple_value<decltype(tc)::value>(ntuple_pack(load_cells(boards + 16 * i)), sh, weights);
    });
    return 0;
}

// ntuple_search_root of n plain boards: action[n], value[n][4]; -1 for a depth or description out of range
int ntuple_check_search(const uint8_t *boards, uint64_t n, uint32_t depth, const Desc *d, const int32_t *weights, uint8_t *action,
                        int64_t *value)
{
    if (!desc_ok(d, kMaxKind) || depth < 1 || depth > kNtupleSearchMaxDepth)
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        for (uint64_t i = 0; i < n; ++i) {
            const Board b = load_cells(boards + 16 * i);
            action[i] = static_cast<uint8_t>(depth == 1 ? ntuple_search_root<1, T>(b, sh, d->F, weights, HostTables(), value + 4 * i)
                                                        : ntuple_search_root<2, T>(b, sh, d->F, weights, HostTables(), value + 4 * i));
        }
    });
    return 0;
}

// The search kernel's split on one thread: sum[n][4] = the sum over sub < K of ntuple_chance_partial(a_d, sub, K) (0 where
// d is illegal) -- for K = 1 the one-thread chance sum, before the division.
int ntuple_check_chance_split(const uint8_t *boards, uint64_t n, uint32_t depth, const Desc *d, const int32_t *weights, uint32_t K,
                              int64_t *sum)
{
    if (!desc_ok(d, kMaxKind) || depth < 1 || depth > kNtupleSearchMaxDepth || K < 1)
        return -1;
    const HostTables tb;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t dir = 0; dir < 4; ++dir) {
                Board a = load_cells(boards + 16 * i);
                uint32_t gain;
                sum[4 * i + dir] = 0;
                if (move_sel(a, tb.move_sel(dir), gain))
                    for (uint32_t sub = 0; sub < K; ++sub)
                        sum[4 * i + dir] += depth == 1 ? ntuple_chance_partial<1, T>(a, sub, K, sh, d->F, weights, tb)
                                                       : ntuple_chance_partial<2, T>(a, sub, K, sh, d->F, weights, tb);
            }
    });
    return 0;
}

// ------------------------------------------------------------------------------------------------ updates
// The one-step update of n boards, in place; mode as update_items takes it.  -1 for an argument out of range.
int ntuple_check_update(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t mode, const Desc *d,
                        int32_t *weights, int64_t *err, int64_t *mag)
{
    return update_items(NtupleBoardItems{as_boards(boards), static_cast<uint32_t>(n)}, delta, lr_shift, mode, d, weights, err, mag);
}

// the entry point of the TC tests: phases 1..3 only
int ntuple_check_tc_update(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases, const Desc *d,
                           int32_t *weights, int64_t *err, int64_t *mag)
{
    return phases >= 1 ? ntuple_check_update(boards, n, delta, lr_shift, phases, d, weights, err, mag) : -1;
}

// push into `slot`, in place on hist / len, writing delta; -1 for H or slot out of range
int ntuple_check_push(const uint8_t *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated, uint64_t n,
                      uint32_t H, uint8_t *hist, uint8_t *len, uint32_t slot, int64_t *delta)
{
    if (H < 1 || H > kNtupleTraceMax || slot >= H)
        return -1;
    for (uint64_t i = 0; i < n; ++i) {
        const bool term = terminated[i] != 0;
        memcpy(hist + (static_cast<uint64_t>(slot) * n + i) * 16, after + 16 * i, 16);
        delta[i] = ntuple_trace_delta(best_next[i], after_value[i], term);
        len[i] = static_cast<uint8_t>(ntuple_trace_push_len(len[i], H, term));
    }
    return 0;
}

// The trace update of n boards, in place, in the kernels' item order; mode as above.  -1 for an argument out of range.
int ntuple_check_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t mode, const Desc *d, int32_t *weights,
                              int64_t *err, int64_t *mag, uint32_t H, uint32_t lam, const uint8_t *hist, const uint8_t *len,
                              uint32_t slot)
{
    if (H < 1 || H > kNtupleTraceMax || lam > kNtupleTcOne || slot >= H)
        return -1;
    return update_items(NtupleTraceItems{as_boards(hist), len, static_cast<uint32_t>(n), H, lam, slot}, delta, lr_shift, mode, d, weights,
                        err, mag);
}

} // extern "C"
