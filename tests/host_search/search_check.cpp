// search_check.cpp -- TEST HARNESS ONLY: the expectimax code of g2048_device.h compiled with g++ (-DG2048_HOST_CHECK),
// one board at a time on one thread.  tests/test_search_host.py compares it with the pure-Python reference
// (tests/search_ref.py), the GPU tests compare the kernels with it, and tools/search_probe.py times it as the host
// baseline.  Not part of the product.
#define G2048_HOST_CHECK 1
#include "../../gym-2048_amd/csrc/g2048_device.h"

#include <cstring>

using namespace g2048;

namespace {

const uint32_t kLut[32] = {G2048_MOVE_LUT_WORDS};

struct HostTables { // what LdsTables is on the device (g2048_kernels.hip)
    MoveSel move_sel(uint32_t m) const
    {
        const uint32_t *r = kLut + 8 * (m & 3u);
        return MoveSel{r[0], r[1], r[2], r[3], r[4], r[5]};
    }
};

Board load_cells(const uint8_t *b)
{
    Board bd;
    std::memcpy(bd.r, b, 16);
    for (int i = 0; i < 4; ++i)
        bd.r[i] &= kCellBits; // exponents mod 32, as the plain kernels read them
    return bd;
}

SearchWeights weights(const int32_t w[4])
{
    return SearchWeights{(uint32_t)w[0], (uint32_t)w[1], (uint32_t)w[2], (uint32_t)w[3]};
}

template <int D> uint32_t root(const Board &b, const SearchWeights &w, int32_t value[4])
{
    return search_root<D>(b, w, HostTables(), value);
}

// the kernels' split: K lanes per direction, each summing its own chance items, then one sum and one divide
template <int D> void root_split(const Board &b, const SearchWeights &w, uint32_t K, int32_t value[4])
{
    for (uint32_t m = 0; m < 4; ++m) {
        Board a = b;
        uint32_t gain;
        if (!move_sel(a, HostTables().move_sel(m), gain)) {
            value[m] = -1;
            continue;
        }
        uint64_t sum = 0;
        for (uint32_t sub = 0; sub < K; ++sub)
            sum += chance_partial<D>(a, sub, K, w, HostTables());
        value[m] = (int32_t)(sum / (10u * count_empty(a)));
    }
}

// number of heuristic evaluations (leaves) of V_D(b), mirroring search_value / chance_partial
template <int D> uint64_t leaves_value(const Board &b)
{
    if constexpr (D == 0) {
        return 1;
    } else {
        uint64_t total = 0;
        for (uint32_t m = 0; m < 4; ++m) {
            Board a = b;
            uint32_t gain;
            if (move_sel(a, HostTables().move_sel(m), gain))
                for (uint32_t e = empty_bits(a); e; e &= e - 1)
                    for (uint32_t v = 1; v <= 2; ++v)
                        total += leaves_value<D - 1>(place(a, g2048_ctz(e), v));
        }
        return total;
    }
}

} // namespace

extern "C" {

// total leaves of a depth-`depth` search over n boards (the root is V_depth without its max)
uint64_t search_check_leaves(const uint8_t *boards, uint64_t n, uint32_t depth)
{
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const Board b = load_cells(boards + 16 * i);
        total += depth == 1 ? leaves_value<1>(b) : depth == 2 ? leaves_value<2>(b) : leaves_value<3>(b);
    }
    return total;
}

uint32_t search_check_heuristic(const uint8_t board[16], const int32_t w[4])
{
    return heuristic(load_cells(board), weights(w));
}

// action[n] and value[n][4] of g2048_expectimax_plain; returns 0, or -1 for a depth outside 1..3
int search_check_boards(const uint8_t *boards, uint64_t n, uint32_t depth, const int32_t w[4], uint8_t *action,
                        int32_t *value)
{
    if (depth < 1 || depth > 3)
        return -1;
    const SearchWeights sw = weights(w);
    for (uint64_t i = 0; i < n; ++i) {
        const Board b = load_cells(boards + 16 * i);
        int32_t *v = value + 4 * i;
        action[i] = (uint8_t)(depth == 1 ? root<1>(b, sw, v) : depth == 2 ? root<2>(b, sw, v) : root<3>(b, sw, v));
    }
    return 0;
}

// the root values through the kernels' lane split with K lanes per direction
int search_check_split(const uint8_t *boards, uint64_t n, uint32_t depth, const int32_t w[4], uint32_t K, int32_t *value)
{
    if (depth < 1 || depth > 3 || K == 0)
        return -1;
    const SearchWeights sw = weights(w);
    for (uint64_t i = 0; i < n; ++i) {
        const Board b = load_cells(boards + 16 * i);
        int32_t *v = value + 4 * i;
        if (depth == 1)
            root_split<1>(b, sw, K, v);
        else if (depth == 2)
            root_split<2>(b, sw, K, v);
        else
            root_split<3>(b, sw, K, v);
    }
    return 0;
}

} // extern "C"
