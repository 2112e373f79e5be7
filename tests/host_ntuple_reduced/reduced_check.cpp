// reduced_check.cpp -- the n-tuple reduced search of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK): a one-thread root written here as the plain recursion of the definition over the header's move, chance
// item and look-up code (S^R_k for any k, nothing of the kernel's steps), and the split of ntuple_reduced_search_kernel -- the
// depth of a board from its empty cells and the schedule, then root, [leaves1 | expand, scan, leaves, fold], finish over an
// NtupleDeepLds -- run by P simulated lanes, each step for every lane before the next step begins (the kernel's barriers), with
// plain adds where the kernel uses LDS atomics.  For uniform, staged and mixed-length networks.
// tests/test_ntuple_reduced_host.py compares both with the pure-Python reference, with the composition by definition and with
// each other.  Not part of the product.
#include "../host_common/ntuple_host.h"

namespace {

// S^R_k(b) by the definition, recursively (host only): the children of a 4 spawn R plies shallower
template <uint32_t T, class Shape>
int64_t state_value(const Board &b, uint32_t k, uint32_t R, const Shape &sh, uint32_t F, const int32_t *weights);

template <uint32_t T, class Shape>
int64_t after_value(const Board &a, uint32_t k, uint32_t R, const Shape &sh, uint32_t F, const int32_t *weights)
{
    if (k == 0u)
        return ntuple_value<T>(ntuple_pack(a), sh, weights);
    int64_t sum = 0;
    chance_items(a, 0u, 1u, [&](const Board &child, uint32_t weight) {
        const uint32_t less = weight == 9u ? 1u : 1u + R;
        sum += static_cast<int64_t>(weight) * state_value<T>(child, k > less ? k - less : 0u, R, sh, F, weights);
    });
    return floor_div(sum, 10 * static_cast<int64_t>(count_empty(a)));
}

template <uint32_t T, class Shape>
int64_t state_value(const Board &b, uint32_t k, uint32_t R, const Shape &sh, uint32_t F, const int32_t *weights)
{
    const HostTables tb;
    int64_t best = 0;
    bool any = false;
    for (uint32_t m = 0; m < 4u; ++m) {
        Board a = b;
        uint32_t gain;
        if (move_sel(a, tb.move_sel(m), gain)) {
            const int64_t q = static_cast<int64_t>(static_cast<uint64_t>(gain) << F) + after_value<T>(a, k, R, sh, F, weights);
            best = !any || q > best ? q : best;
            any = true;
        }
    }
    return best;
}

template <uint32_t T, class Shape>
uint32_t reduced_root(const Board &cells, uint32_t depth, uint32_t R, const Shape &sh, uint32_t F, const int32_t *weights, int64_t value[4])
{
    const HostTables tb;
    uint64_t best = 0;
    for (uint32_t d = 0; d < 4u; ++d) {
        Board a = cells;
        uint32_t gain;
        const bool legal = move_sel(a, tb.move_sel(d), gain);
        value[d] = legal ? static_cast<int64_t>(static_cast<uint64_t>(gain) << F) + after_value<T>(a, depth, R, sh, F, weights) : kNtupleIllegal;
        const uint64_t key = ntuple_key(value[d], legal, d);
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
uint32_t split_board(NtupleDeepLds &l, const Board &cells, bool active, uint32_t depth, uint32_t R, uint32_t P, const Shape &sh, uint32_t F,
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
        all_lanes(P, [&](uint32_t lane) { ntuple_reduced_expand(l, depth, R, lane, P, tb); });
        all_lanes(P, [&](uint32_t lane) { ntuple_deep_scan(l, lane, P); });
        all_lanes(P, [&](uint32_t lane) {
            ntuple_reduced_leaves<T>(l, depth, R, lane, P, sh, F, weights, tb, [&l](uint32_t e, int64_t x) {
                l.acc[e] = static_cast<long long>(static_cast<uint64_t>(l.acc[e]) + static_cast<uint64_t>(x));
            });
        });
        all_lanes(P, [&](uint32_t lane) { ntuple_reduced_fold(l, lane, P, F, add_root); });
    }
    return ntuple_adaptive_finish(l, depth, F, value);
}

bool reduce_ok(uint32_t R) { return R >= kNtupleReduce4Min && R <= kNtupleReduce4Max; }

} // namespace

extern "C" {

// The one-thread root of n plain boards at one depth 0..4: action[n], value[n][4]; -1 for an argument out of range
int reduced_check_root(const uint8_t *boards, uint64_t n, uint32_t depth, uint32_t R, const Desc *d, const int32_t *weights,
                       uint8_t *action, int64_t *value)
{
    if (!desc_ok(d, 2) || depth > kNtupleAdaptiveMaxDepth || !reduce_ok(R))
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        for (uint64_t i = 0; i < n; ++i)
            action[i] = static_cast<uint8_t>(reduced_root<T>(load_cells(boards + 16 * i), depth, R, sh, d->F, weights, value + 4 * i));
    });
    return 0;
}

// S^R_k of n plain boards, k in 0..2, by the tree a lane of the kernel runs for a work unit (ntuple_reduced_state): value[n]
int reduced_check_unit(const uint8_t *boards, uint64_t n, uint32_t k, const Desc *d, const int32_t *weights, int64_t *value)
{
    if (!desc_ok(d, 2) || k > 2u)
        return -1;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        const HostTables tb;
        for (uint64_t i = 0; i < n; ++i)
            value[i] = ntuple_reduced_state<T>(load_cells(boards + 16 * i), k, sh, d->F, weights, tb);
    });
    return 0;
}

// The reduced kernel's split of n plain boards with P lanes under schedule[17] and R: action[n], value[n][4], depth[n] as the
// kernel writes them.  active NULL or uint32[n].  -1 for an argument out of range.
int reduced_check_split(const uint8_t *boards, uint64_t n, const uint8_t *schedule, uint32_t R, const Desc *d, const int32_t *weights,
                        uint32_t P, const uint32_t *active, uint8_t *action, int64_t *value, uint8_t *depth)
{
    if (!desc_ok(d, 2) || !schedule || P < 1 || !reduce_ok(R))
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
            action[i] = static_cast<uint8_t>(split_board<T>(*l, b, on, D, R, P, sh, d->F, weights, value + 4 * i));
            depth[i] = static_cast<uint8_t>(on ? D : kNtupleAdaptiveSkipped);
        }
        delete l;
    });
    return 0;
}

} // extern "C"
