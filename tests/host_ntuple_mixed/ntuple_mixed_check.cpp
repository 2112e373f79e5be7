// ntuple_mixed_check.cpp -- the mixed-length n-tuple code of g2048_device.h (NtupleMixedShape: the header the kernels are
// compiled from) built for the host (-DG2048_HOST_CHECK) on one thread: values, evaluate, search, the TD, TC and trace
// updates, staged or not, and the offsets of every look-up.  The updates run the header's item sources, item loop and
// per-item operations -- what the update kernels run -- with wrapping adds for the atomic ones.
// tests/test_ntuple_mixed_host.py compares it with tests/ntuple_mixed_ref.py.  Not part of the product.
#include "../host_common/ntuple_host.h"

namespace {

// every call here instantiates NtupleMixedShape, whatever the lengths of the lists: kind 2 alone
bool mixed_ok(const Desc *d) { return desc_ok(d, 2) && d->kind == 2; }

NtupleMixedShape shape_of(const Desc *d) { return ntuple_mixed_shape(d->T, d->L, d->cells, d->S, d->thr); }

template <class Items>
int update_items(const Items &items, const int64_t *delta, uint32_t lr_shift, uint32_t mode, const Desc *d, int32_t *weights, int64_t *err,
                 int64_t *mag)
{
    if (!mixed_ok(d) || lr_shift > kNtupleMaxShift || mode > 3)
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

// the shape's own numbers: is_mixed, W, len[8] (from the list words' top byte), base[8]
int ntuple_mixed_check_shape(const Desc *d, uint32_t *is_mixed, uint32_t *n_weights, uint32_t *len, uint32_t *base)
{
    if (!mixed_ok(d))
        return -1;
    const NtupleMixedShape sh = shape_of(d);
    *is_mixed = ntuple_is_mixed(d->T, d->L, d->cells) ? 1u : 0u;
    *n_weights = sh.n_weights;
    for (uint32_t t = 0; t < d->T; ++t) {
        len[t] = sh.list[t] >> 26; // 4 * L_t in bits 24..31
        base[t] = sh.base[t];
    }
    return 0;
}

// the element every look-up reads: out[n][8][T] = ntuple_offset(packed, sh, s, t, ntuple_stage_base(packed, sh))
int ntuple_mixed_check_offsets(const uint8_t *boards, uint64_t n, const Desc *d, uint32_t *out)
{
    if (!mixed_ok(d))
        return -1;
    const NtupleMixedShape sh = shape_of(d);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t packed = ntuple_pack(load_cells(boards + 16 * i));
        const uint32_t base = ntuple_stage_base(packed, sh);
        for (uint32_t s = 0; s < 8u; ++s)
            for (uint32_t t = 0; t < d->T; ++t)
                *out++ = ntuple_offset(packed, sh, s, t, base);
    }
    return 0;
}

int ntuple_mixed_check_values(const uint8_t *boards, uint64_t n, const Desc *d, const int32_t *weights, int64_t *v)
{
    if (!mixed_ok(d))
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
        for (uint64_t i = 0; i < n; ++i)
            v[i] = ntuple_value<decltype(tc)::value>(ntuple_pack(load_cells(boards + 16 * i)), sh, weights);
    });
    return 0;
}

int ntuple_mixed_check_evaluate(const uint8_t *boards, uint64_t n, const Desc *d, const int32_t *weights, int64_t *value, uint8_t *action,
                                int64_t *best, uint8_t *after, int64_t *after_value)
{
    if (!mixed_ok(d))
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

int ntuple_mixed_check_search(const uint8_t *boards, uint64_t n, uint32_t depth, const Desc *d, const int32_t *weights, uint8_t *action,
                              int64_t *value)
{
    if (!mixed_ok(d) || depth < 1 || depth > kNtupleSearchMaxDepth)
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

// The one-step update of n boards, in place.  mode 0: the TD update; 1..3: the TC update with those phases.
int ntuple_mixed_check_update(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t mode, const Desc *d,
                              int32_t *weights, int64_t *err, int64_t *mag)
{
    return update_items(NtupleBoardItems{as_boards(boards), static_cast<uint32_t>(n)}, delta, lr_shift, mode, d, weights, err, mag);
}

// The trace update of n boards, in place, in the kernels' item order; mode as above.
int ntuple_mixed_check_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t mode, const Desc *d, int32_t *weights,
                                    int64_t *err, int64_t *mag, uint32_t H, uint32_t lam, const uint8_t *hist, const uint8_t *len,
                                    uint32_t slot)
{
    if (H < 1 || H > kNtupleTraceMax || lam > kNtupleTcOne || slot >= H)
        return -1;
    return update_items(NtupleTraceItems{as_boards(hist), len, static_cast<uint32_t>(n), H, lam, slot}, delta, lr_shift, mode, d, weights,
                        err, mag);
}

} // extern "C"
