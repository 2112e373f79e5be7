// deep_check.cpp -- the n-tuple deep search of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK): ntuple_search_root<D> on one thread for D = 1..3, and the split of ntuple_deep_search_kernel -- root,
// expand, scan, leaves, fold, finish over an NtupleDeepLds -- run by P simulated lanes, each step for every lane before the
// next step begins (the kernel's barriers), with plain adds where the kernel uses LDS atomics.  For uniform, staged and
// mixed-length networks.  tests/test_ntuple_deep_host.py compares both with tests/ntuple_search_ref.py and with each other.
// -DDEEP_CHECK_MAIN adds a stand-alone main() that runs the split against the one-thread root on a fixed board set (the
// form a sanitizer build runs).  Not part of the product.
#include "../host_common/ntuple_host.h"

namespace {

// One board through the kernel's steps with P lanes; the table is the caller's (the kernel reuses its LDS from board to board)
template <int D, uint32_t T, class Shape>
uint32_t split_board(NtupleDeepLds &l, const Board &cells, bool active, uint32_t P, const Shape &sh, uint32_t F, const int32_t *weights,
                     int64_t value[4])
{
    const HostTables tb;
    for (uint32_t lane = 0; lane < P; ++lane)
        ntuple_deep_root(l, cells, active, lane, tb);
    if (P < 4u) // (the kernel has 256 lanes; fewer simulated lanes take the root directions in turn)
        for (uint32_t lane = P; lane < 4u; ++lane)
            ntuple_deep_root(l, cells, active, lane, tb);
    for (uint32_t lane = 0; lane < P; ++lane)
        ntuple_deep_expand(l, lane, P, tb);
    for (uint32_t lane = 0; lane < P; ++lane)
        ntuple_deep_scan(l, lane, P);
    for (uint32_t lane = 0; lane < P; ++lane)
        ntuple_deep_leaves<D, T>(l, lane, P, sh, F, weights, tb, [&l](uint32_t e, int64_t x) {
            l.acc[e] = static_cast<long long>(static_cast<uint64_t>(l.acc[e]) + static_cast<uint64_t>(x));
        });
    for (uint32_t lane = 0; lane < P; ++lane)
        ntuple_deep_fold(l, lane, P, F, [&l](uint32_t d1, int64_t x) {
            l.root_sum[d1] = static_cast<long long>(static_cast<uint64_t>(l.root_sum[d1]) + static_cast<uint64_t>(x));
        });
    return ntuple_deep_finish(l, F, value);
}

} // namespace

extern "C" {

// ntuple_search_root<depth> of n plain boards on one thread: action[n], value[n][4]; -1 for an argument out of range
int deep_check_root(const uint8_t *boards, uint64_t n, uint32_t depth, const Desc *d, const int32_t *weights, uint8_t *action,
                    int64_t *value)
{
    if (!desc_ok(d, 2) || depth < 1 || depth > kNtupleDeepMaxDepth)
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        const HostTables tb;
        for (uint64_t i = 0; i < n; ++i) {
            const Board b = load_cells(boards + 16 * i);
            int64_t *v = value + 4 * i;
            action[i] = static_cast<uint8_t>(depth == 1   ? ntuple_search_root<1, T>(b, sh, d->F, weights, tb, v)
                                             : depth == 2 ? ntuple_search_root<2, T>(b, sh, d->F, weights, tb, v)
                                                          : ntuple_search_root<3, T>(b, sh, d->F, weights, tb, v));
        }
    });
    return 0;
}

// The deep search kernel's split of n plain boards with P lanes: action[n], value[n][4], and, where they are not NULL,
// items[n] = the level-1 items of the board and units[n] = its work units.  active NULL or uint32[n].  -1 for an argument
// out of range.
int deep_check_split(const uint8_t *boards, uint64_t n, uint32_t depth, const Desc *d, const int32_t *weights, uint32_t P,
                     const uint32_t *active, uint8_t *action, int64_t *value, uint32_t *items, uint32_t *units)
{
    if (!desc_ok(d, 2) || depth < kNtupleDeepMinDepth || depth > kNtupleDeepMaxDepth || P < 1)
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        NtupleDeepLds *l = new NtupleDeepLds;
        memset(l, 0xA5, sizeof(*l)); // whatever a step reads, a step before it has written
        for (uint64_t i = 0; i < n; ++i) {
            const Board b = load_cells(boards + 16 * i);
            const bool on = !active || active[i] != 0u;
            action[i] = static_cast<uint8_t>(depth == 2 ? split_board<2, T>(*l, b, on, P, sh, d->F, weights, value + 4 * i)
                                                        : split_board<3, T>(*l, b, on, P, sh, d->F, weights, value + 4 * i));
            if (items)
                items[i] = ntuple_deep_items(*l);
            if (units)
                units[i] = l->first[4u * ntuple_deep_items(*l)];
        }
        delete l;
    });
    return 0;
}

uint32_t deep_check_lds_bytes() { return static_cast<uint32_t>(sizeof(NtupleDeepLds)); }

} // extern "C"

#ifdef DEEP_CHECK_MAIN
#include <cstdio>
#include <vector>

// The split against the one-thread root, depth 2 and 3, P in {1, 64, 256}, on a fixed set: near-full boards, a board with no
// move, sparse boards (wide fans) at depth 2, and a one-tuple and a four-tuple network with weights from an LCG.
int main()
{
    const uint8_t fixed[][16] = {
        {1, 1, 3, 2, 5, 6, 7, 4, 1, 2, 3, 5, 4, 5, 6, 7},  // two legal moves, one empty cell after either
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1},  // no legal move
        {1, 2, 3, 4, 2, 3, 4, 5, 3, 4, 5, 6, 0, 5, 6, 7},  // one empty cell
        {1, 2, 3, 4, 2, 3, 4, 5, 3, 4, 5, 6, 0, 0, 6, 7},  // two
        {2, 2, 3, 4, 0, 3, 3, 5, 3, 0, 5, 5, 0, 5, 6, 6},  // three, merges everywhere
        {15, 16, 17, 31, 2, 3, 4, 5, 3, 4, 5, 6, 0, 5, 31, 31}, // at and past the clamp
    };
    const uint8_t sparse[][16] = {
        {0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},  // one tile: 30 items in every direction
        {1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
        {1, 2, 3, 4, 2, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    };
    std::vector<int32_t> weights(3u * 4u << 16); // [S][T][16^L] of the larger network
    uint32_t x = 12345u;
    for (int32_t &w : weights) {
        x = x * 1664525u + 1013904223u;
        w = static_cast<int32_t>(x);
    }
    const Desc nets[2] = {{1, 4, 10, 1, 0, {}, {{0, 1, 4, 5}}},
                          {4, 4, 16, 3, 1, {4, 24}, {{0, 1, 2, 3}, {4, 5, 6, 7}, {0, 1, 4, 5}, {5, 6, 9, 10}}}};
    int bad = 0;
    for (const Desc &d : nets)
        for (uint32_t depth = 2; depth <= 3; ++depth) {
            std::vector<uint8_t> boards(&fixed[0][0], &fixed[0][0] + sizeof(fixed));
            if (depth == 2)
                boards.insert(boards.end(), &sparse[0][0], &sparse[0][0] + sizeof(sparse));
            const uint64_t n = boards.size() / 16;
            std::vector<uint8_t> want_a(n), got_a(n);
            std::vector<int64_t> want_v(4 * n), got_v(4 * n);
            if (deep_check_root(boards.data(), n, depth, &d, weights.data(), want_a.data(), want_v.data()) != 0)
                return 2;
            for (uint32_t P : {1u, 64u, 256u}) {
                if (deep_check_split(boards.data(), n, depth, &d, weights.data(), P, nullptr, got_a.data(), got_v.data(), nullptr, nullptr) != 0)
                    return 2;
                const bool same = got_a == want_a && got_v == want_v;
                printf("T=%u depth=%u P=%u boards=%llu: %s\n", d.T, depth, P, static_cast<unsigned long long>(n), same ? "equal" : "DIFFERENT");
                bad += same ? 0 : 1;
            }
        }
    return bad ? 1 : 0;
}
#endif
