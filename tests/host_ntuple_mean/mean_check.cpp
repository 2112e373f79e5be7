// mean_check.cpp -- the batch-mean update of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK) on one thread: the header's item sources and its two per-item operations, ntuple_item_mean_sum and
// ntuple_item_mean_apply -- what the two kernels run -- with plain adds for the atomic adds and a plain read-then-zero for the
// atomic exchanges, over any of the three shape types and in any item order.
// tests/test_ntuple_mean_host.py compares it with tests/ntuple_mean_ref.py.  Not part of the product.
#include "../host_common/ntuple_host.h"

namespace {

// f(item) for every item of a source: through the header's loop, or in the caller's order (a permutation of 0..size-1)
template <class Items, class F> bool visit(const Items &items, const uint64_t *order, uint64_t n_order, F f)
{
    if (!order) {
        ntuple_for_items(items, 0, 1, f);
        return true;
    }
    if (n_order != items.size())
        return false;
    for (uint64_t k = 0; k < n_order; ++k) {
        if (order[k] >= items.size())
            return false;
        f(items.at(order[k]));
    }
    return true;
}

template <class Items>
int update_items(const Items &items, const int64_t *delta, uint32_t lr_shift, uint32_t phases, const Desc *d, int32_t *weights, int64_t *sum,
                 uint32_t *count, const uint64_t *order, uint64_t n_order)
{
    if (!desc_ok(d, 2) || lr_shift > kNtupleMaxShift || phases < 1 || phases > 3 || items.size() >= (1ull << 29))
        return -1;
    uint32_t *w = reinterpret_cast<uint32_t *>(weights);
    uint64_t *s = reinterpret_cast<uint64_t *>(sum);
    auto add_sum = [s, count](uint32_t off, int64_t dd) {
        s[off] += static_cast<uint64_t>(dd);
        count[off] += 1u;
    };
    auto claim = [count](uint32_t off) {
        const uint32_t c = count[off];
        count[off] = 0;
        return c;
    };
    auto take = [s](uint32_t off) {
        const int64_t a = static_cast<int64_t>(s[off]);
        s[off] = 0;
        return a;
    };
    auto add = [w](uint32_t off, int32_t step) { w[off] += static_cast<uint32_t>(step); };
    using Item = typename Items::Item;
    bool ok = true;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        if (phases & 1u)
            ok = ok && visit(items, order, n_order, [&](Item it) { ntuple_item_mean_sum<T>(items, delta, it, sh, add_sum); });
        if (phases & 2u)
            ok = ok && visit(items, order, n_order, [&](Item it) { ntuple_item_mean_apply<T>(items, delta, it, lr_shift, sh, claim, take, add); });
    });
    return ok ? 0 : -1;
}

const uint4 *as_boards(const uint8_t *p) { return reinterpret_cast<const uint4 *>(p); }

} // namespace

extern "C" {

int mean_check_floor_div(int64_t a, uint32_t c, int64_t *out)
{
    if (c == 0)
        return -1;
    *out = ntuple_mean_floor_div(a, c);
    return 0;
}

// The batch-mean update of n plain boards, in place; phases 1 (SUM), 2 (APPLY) or 3; order: NULL or a permutation of 0..n-1.
int mean_check_update(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases, const Desc *d,
                      int32_t *weights, int64_t *sum, uint32_t *count, const uint64_t *order, uint64_t n_order)
{
    if (n == 0 || n > 0xffffff00ull)
        return -1;
    return update_items(NtupleBoardItems{as_boards(boards), static_cast<uint32_t>(n)}, delta, lr_shift, phases, d, weights, sum, count, order,
                        n_order);
}

// The batch-mean trace update of n boards, in place; order: NULL or a permutation of the H * n item numbers k * n + i.
int mean_check_trace_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases, const Desc *d, int32_t *weights,
                            int64_t *sum, uint32_t *count, uint32_t H, uint32_t lam, const uint8_t *hist, const uint8_t *len, uint32_t slot,
                            const uint64_t *order, uint64_t n_order)
{
    if (n == 0 || n > 0xffffff00ull || H < 1 || H > kNtupleTraceMax || lam > kNtupleTcOne || slot >= H)
        return -1;
    return update_items(NtupleTraceItems{as_boards(hist), len, static_cast<uint32_t>(n), H, lam, slot}, delta, lr_shift, phases, d, weights,
                        sum, count, order, n_order);
}

} // extern "C"
