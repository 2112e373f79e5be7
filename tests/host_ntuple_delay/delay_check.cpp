// delay_check.cpp -- the n-tuple delay of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK) on one thread: the header's push function, and the header's item loop and per-item operations over
// NtupleDelayItems -- what ntuple_delay_push_kernel and the three update kernels run -- with wrapping adds for the atomic
// ones.  The items can be visited in ascending, descending or stride-7 order: the tables must not depend on it.
// tests/test_ntuple_delay_host.py compares it bit for bit with tests/ntuple_delay_ref.py.  With -DDELAY_CHECK_MAIN the file
// is a stand-alone program that runs the same code on generated pushes (for a sanitizer build) and checks what can be
// checked without the reference: the three orders agree, and lambda = 0 equals the plain updates.  Not part of the product.
#include "../host_common/ntuple_host.h"

namespace {

// f(item) for every item of a source.  order 0: ascending, through the header's loop; 1: descending; 2: the residues mod 7
// one after the other, each through the header's loop with stride 7 -- a lane's walk with a grid of 7
template <class Items, class F> void visit(const Items &items, uint32_t order, F f)
{
    if (order == 0)
        ntuple_for_items(items, 0, 1, f);
    else if (order == 1)
        for (uint64_t index = items.size(); index-- > 0;)
            f(items.at(index));
    else
        for (uint64_t first = 0; first < 7; ++first)
            ntuple_for_items(items, 6 - first, 7, f);
}

// The update of every item of a source, in place.  form 0: the TD update; 1..3: the TC update with phases = form, phase W over
// every item, then phase A over every item.
template <class Items>
int update_items(const Items &items, const int64_t *delta, uint32_t lr_shift, uint32_t form, uint32_t order, const Desc *d, int32_t *weights,
                 int64_t *err, int64_t *mag)
{
    if (!desc_ok(d, 2) || lr_shift > kNtupleMaxShift || form > 3 || order > 2)
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
        if (form == 0)
            visit(items, order, [&](Item it) { ntuple_item_update<T>(items, delta, it, lr_shift, sh, add); });
        if (form & 1u)
            visit(items, order, [&](Item it) { ntuple_item_tc_weights<T>(items, delta, it, lr_shift, sh, err, mag, add); });
        if (form & 2u)
            visit(items, order, [&](Item it) { ntuple_item_tc_accum<T>(items, delta, it, sh, accum); });
    });
    return 0;
}

const uint4 *as_boards(const uint8_t *p) { return reinterpret_cast<const uint4 *>(p); }

bool ring_ok(uint32_t H, uint32_t lam, uint32_t slot) { return H >= 1 && H <= kNtupleTraceMax && lam <= kNtupleTcOne && slot < H; }

} // namespace

extern "C" {

// 1 / 0: ntuple_delay_due
uint32_t delay_check_due(uint32_t len, uint32_t k, uint32_t H, uint32_t mode) { return ntuple_delay_due(len, k, H, mode) ? 1u : 0u; }

// delay push into `slot`, in place on hist / len / acc, writing delta; -1 for an argument out of range
int delay_check_push(const uint8_t *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated, uint64_t n,
                     uint32_t H, uint32_t lam, uint8_t *hist, uint8_t *len, int64_t *acc, uint32_t slot, int64_t *delta)
{
    if (!ring_ok(H, lam, slot))
        return -1;
    for (uint64_t i = 0; i < n; ++i) {
        memcpy(hist + (static_cast<uint64_t>(slot) * n + i) * 16, after + 16 * i, 16);
        delta[i] = ntuple_delay_push(len[i], best_next[i], after_value[i], terminated[i] != 0, lam, slot, H,
                                     [&](uint32_t plane) -> int64_t & { return acc[static_cast<uint64_t>(plane) * n + i]; });
    }
    return 0;
}

// The delay update of n boards, in place; form and order as above, mode kNtupleDelayStep or kNtupleDelayFlush.
int delay_check_update(uint64_t n, uint32_t lr_shift, uint32_t form, uint32_t mode, uint32_t order, const Desc *d, int32_t *weights,
                       int64_t *err, int64_t *mag, uint32_t H, const uint8_t *hist, const uint8_t *len, const int64_t *acc, uint32_t slot)
{
    if (!ring_ok(H, 0, slot) || mode > kNtupleDelayFlush)
        return -1;
    return update_items(NtupleDelayItems{as_boards(hist), len, static_cast<uint32_t>(n), H, slot, mode}, acc, lr_shift, form, order, d,
                        weights, err, mag);
}

// The one-step update of n boards, in place (NtupleBoardItems): what lambda = 0 must add up to.
int delay_check_plain_update(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t form, const Desc *d,
                             int32_t *weights, int64_t *err, int64_t *mag)
{
    return update_items(NtupleBoardItems{as_boards(boards), static_cast<uint32_t>(n)}, delta, lr_shift, form, 0, d, weights, err, mag);
}

} // extern "C"

#ifdef DELAY_CHECK_MAIN
#include <cstdio>
#include <vector>

namespace {

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

const uint8_t kCells[8][6] = {{0, 1, 2, 3, 4, 5}, {4, 5, 6, 7, 8, 9}, {0, 1, 2, 4, 5, 6}, {4, 5, 6, 8, 9, 10},
                              {0, 4, 8, 12, 13, 9}, {3, 2, 1, 5, 9, 13}, {15, 14, 10, 11, 7, 6}, {12, 8, 9, 5, 6, 2}};

Desc make_desc(uint32_t T, uint32_t kind)
{
    Desc d{};
    d.T = T;
    d.L = 4;
    d.F = 10;
    d.S = kind == 0 ? 1 : 3;
    d.kind = kind;
    d.thr[0] = 1u << 3; // a board that holds an 8
    d.thr[1] = 1u << 6;
    for (uint32_t t = 0; t < T; ++t)
        for (uint32_t k = 0; k < 4; ++k)
            d.cells[t][k] = kind == 2 && k > t % 4 ? kNtupleEnd : kCells[t][k]; // mixed: lengths 1, 2, 3, 4, 1, ...
    return d;
}

struct Tables {
    std::vector<int32_t> w;
    std::vector<int64_t> err, mag;
    bool operator==(const Tables &o) const { return w == o.w && err == o.err && mag == o.mag; }
};

// pushes with a STEP update after each, then the FLUSH; form 0, or 1 and 2 as separate calls (W everywhere, then A)
int run(const Desc &d, uint32_t n, uint32_t H, uint32_t lam, uint32_t pushes, uint32_t tc, uint32_t order, Tables &tb, Tables *plain)
{
    std::vector<uint8_t> hist(static_cast<size_t>(H) * n * 16), len(n), after(n * 16), term(n);
    std::vector<int64_t> acc(static_cast<size_t>(H) * n), av(n), best(n), delta(n);
    g_rng = 0x9e3779b97f4a7c15ull + n + H;
    uint32_t slot = H - 1;
    auto update = [&](uint32_t mode) {
        if (!tc)
            return delay_check_update(n, 3, 0, mode, order, &d, tb.w.data(), tb.err.data(), tb.mag.data(), H, hist.data(), len.data(),
                                      acc.data(), slot);
        int rc = delay_check_update(n, 3, 1, mode, order, &d, tb.w.data(), tb.err.data(), tb.mag.data(), H, hist.data(), len.data(),
                                    acc.data(), slot);
        return rc ? rc : delay_check_update(n, 3, 2, mode, order, &d, tb.w.data(), tb.err.data(), tb.mag.data(), H, hist.data(),
                                            len.data(), acc.data(), slot);
    };
    for (uint32_t t = 0; t < pushes; ++t) {
        for (uint32_t i = 0; i < n; ++i) {
            for (uint32_t c = 0; c < 16; ++c)
                after[16 * i + c] = static_cast<uint8_t>(rnd() % 9);
            av[i] = static_cast<int64_t>(rnd() >> 28) - (1ll << 35);
            best[i] = static_cast<int64_t>(rnd() >> 28) - (1ll << 35);
            term[i] = rnd() % 5 == 0 && i % 7 != 6;
        }
        slot = (slot + 1) % H;
        if (delay_check_push(after.data(), av.data(), best.data(), term.data(), n, H, lam, hist.data(), len.data(), acc.data(), slot,
                             delta.data()))
            return -1;
        if (plain && delay_check_plain_update(after.data(), n, delta.data(), 3, 0, &d, plain->w.data(), plain->err.data(), plain->mag.data()))
            return -1;
        if (update(kNtupleDelayStep))
            return -1;
    }
    return update(kNtupleDelayFlush);
}

} // namespace

int main()
{
    int bad = 0, cases = 0;
    for (uint32_t kind = 0; kind < 3; ++kind)
        for (uint32_t T : {1u, 4u, 8u})
            for (uint32_t H : {1u, 3u, 8u})
                for (uint32_t tc = 0; tc < 2; ++tc) {
                    const Desc d = make_desc(T, kind);
                    const size_t size = static_cast<size_t>(d.S) * T * 65536; // an upper bound for the mixed network
                    Tables zero{std::vector<int32_t>(size), std::vector<int64_t>(size), std::vector<int64_t>(size)};
                    Tables got[3] = {zero, zero, zero}, lam0 = zero, plain = zero;
                    for (uint32_t order = 0; order < 3; ++order)
                        if (run(d, 67, H, 40000, 19, tc, order, got[order], nullptr))
                            return printf("case refused\n"), 2;
                    const bool same = got[0] == got[1] && got[0] == got[2] && !(got[0] == zero);
                    bool c3 = true;
                    if (!tc) { // consequence 3
                        if (run(d, 67, H, 0, 19, 0, 2, lam0, &plain))
                            return printf("case refused\n"), 2;
                        c3 = lam0 == plain && !(plain == zero);
                    }
                    ++cases;
                    if (!same || !c3) {
                        ++bad;
                        printf("kind %u T %u H %u tc %u: orders %s, lambda 0 %s\n", kind, T, H, tc, same ? "equal" : "DIFFER", c3 ? "equal" : "DIFFERS");
                    }
                }
    printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
