// adaptive_check.cpp -- the n-tuple adaptive search of g2048_device.h (the header the kernels are compiled from) built for the
// host (-DG2048_HOST_CHECK): the one-thread root at a given depth 0..4 (evaluate's definition at 0, ntuple_search_root<D> above),
// and the split of ntuple_adaptive_search_kernel -- the depth of a board from its empty cells and the schedule, then root,
// [leaves1 | expand, scan, leaves, fold], finish over an NtupleDeepLds -- run by P simulated lanes, each step for every lane
// before the next step begins (the kernel's barriers), with plain adds where the kernel uses LDS atomics.  For uniform, staged
// and mixed-length networks.  tests/test_ntuple_adaptive_host.py compares both with the pure-Python reference, with the
// composition by definition and with each other.  Not part of the product.
#include "../host_common/ntuple_host.h"

namespace {

// evaluate's definition on one thread: q[4] and the action
template <uint32_t T, class Shape>
uint32_t evaluate_root(const Board &cells, const Shape &sh, uint32_t F, const int32_t *weights, int64_t value[4])
{
    const HostTables tb;
    uint64_t best = 0;
    for (uint32_t d = 0; d < 4u; ++d) {
        const NtupleMove m = ntuple_move<T>(cells, d, sh, F, weights, tb);
        value[d] = m.q;
        const uint64_t key = ntuple_key(m.q, m.legal, d);
        best = key > best ? key : best;
    }
    return root_key_action(best);
}

template <class Fn> void all_lanes(uint32_t P, Fn &&fn)
{
    for (uint32_t lane = 0; lane < P; ++lane)
        fn(lane);
}

// One board through the kernel's steps with P lanes; the table is the caller's (the kernel reuses its LDS from board to board)
template <uint32_t T, class Shape>
uint32_t split_board(NtupleDeepLds &l, const Board &cells, bool active, uint32_t depth, uint32_t P, const Shape &sh, uint32_t F,
                     const int32_t *weights, int64_t value[4])
{
    const HostTables tb;
    const auto add_root = [&l](uint32_t d1, int64_t x) {
        l.root_sum[d1] = static_cast<long long>(static_cast<uint64_t>(l.root_sum[d1]) + static_cast<uint64_t>(x));
    };
    // (the kernel has 256 lanes; fewer than four simulated lanes take the root directions in turn)
    all_lanes(P < 4u ? 4u : P, [&](uint32_t lane) { ntuple_adaptive_root<T>(l, cells, active, depth, lane, sh, weights, tb); });
    if (depth == 1u) {
        all_lanes(P, [&](uint32_t lane) { ntuple_adaptive_leaves1<T>(l, lane, P, sh, F, weights, tb, add_root); });
    } else if (depth >= 2u) {
        all_lanes(P, [&](uint32_t lane) { ntuple_deep_expand(l, lane, P, tb); });
        all_lanes(P, [&](uint32_t lane) { ntuple_deep_scan(l, lane, P); });
        all_lanes(P, [&](uint32_t lane) {
            ntuple_adaptive_leaves<T>(l, depth, lane, P, sh, F, weights, tb, [&l](uint32_t e, int64_t x) {
                l.acc[e] = static_cast<long long>(static_cast<uint64_t>(l.acc[e]) + static_cast<uint64_t>(x));
            });
        });
        all_lanes(P, [&](uint32_t lane) { ntuple_deep_fold(l, lane, P, F, add_root); });
    }
    return ntuple_adaptive_finish(l, depth, F, value);
}

} // namespace

extern "C" {

// The one-thread root of n plain boards at one depth 0..4: action[n], value[n][4]; -1 for an argument out of range
int adaptive_check_root(const uint8_t *boards, uint64_t n, uint32_t depth, const Desc *d, const int32_t *weights, uint8_t *action,
                        int64_t *value)
{
    if (!desc_ok(d, 2) || depth > kNtupleAdaptiveMaxDepth)
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        const HostTables tb;
        for (uint64_t i = 0; i < n; ++i) {
            const Board b = load_cells(boards + 16 * i);
            int64_t *v = value + 4 * i;
            action[i] = static_cast<uint8_t>(depth == 0   ? evaluate_root<T>(b, sh, d->F, weights, v)
                                             : depth == 1 ? ntuple_search_root<1, T>(b, sh, d->F, weights, tb, v)
                                             : depth == 2 ? ntuple_search_root<2, T>(b, sh, d->F, weights, tb, v)
                                             : depth == 3 ? ntuple_search_root<3, T>(b, sh, d->F, weights, tb, v)
                                                          : ntuple_search_root<4, T>(b, sh, d->F, weights, tb, v));
        }
    });
    return 0;
}

// The adaptive kernel's split of n plain boards with P lanes under schedule[17]: action[n], value[n][4], depth[n] as the kernel
// writes them.  active NULL or uint32[n].  -1 for an argument out of range.
int adaptive_check_split(const uint8_t *boards, uint64_t n, const uint8_t *schedule, const Desc *d, const int32_t *weights, uint32_t P,
                         const uint32_t *active, uint8_t *action, int64_t *value, uint8_t *depth)
{
    if (!desc_ok(d, 2) || !schedule || P < 1)
        return -1;
    for (uint32_t e = 0; e < 17u; ++e)
        if (schedule[e] > kNtupleAdaptiveMaxDepth)
            return -1;
    const NtupleAdaptiveSchedule sc = ntuple_adaptive_schedule(schedule);
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        NtupleDeepLds *l = new NtupleDeepLds;
        memset(l, 0xA5, sizeof(*l)); // whatever a step reads, a step before it has written
        for (uint64_t i = 0; i < n; ++i) {
            const Board b = load_cells(boards + 16 * i);
            const bool on = !active || active[i] != 0u;
            const uint32_t D = ntuple_adaptive_depth(sc, b);
            action[i] = static_cast<uint8_t>(split_board<T>(*l, b, on, D, P, sh, d->F, weights, value + 4 * i));
            depth[i] = static_cast<uint8_t>(on ? D : kNtupleAdaptiveSkipped);
        }
        delete l;
    });
    return 0;
}

} // extern "C"
