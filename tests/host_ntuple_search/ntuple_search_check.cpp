// ntuple_search_check.cpp -- the n-tuple expectimax of g2048_device.h (the header the kernels are compiled from) built
// for the host (-DG2048_HOST_CHECK), one board at a time on one thread.  tests/test_ntuple_search_host.py compares it
// with the pure-Python reference (tests/ntuple_search_ref.py); the GPU tests compare the kernel with that reference too.
// Not part of the product.
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

// f(std::integral_constant<int, D>(), std::integral_constant<uint32_t, T>()) for the run-time D in 1..2 and T in 1..8
template <uint32_t T = 1, class F> bool with_shape(uint32_t depth, uint32_t n_tuples, F &&f)
{
    if constexpr (T > kNtupleMaxTuples) {
        return false;
    } else {
        if (n_tuples == T) {
            if (depth == 1)
                f(std::integral_constant<int, 1>(), std::integral_constant<uint32_t, T>());
            else
                f(std::integral_constant<int, 2>(), std::integral_constant<uint32_t, T>());
            return true;
        }
        return with_shape<T + 1>(depth, n_tuples, f);
    }
}

bool args_ok(uint32_t depth, uint32_t T, uint32_t L, uint32_t F)
{
    return depth >= 1 && depth <= kNtupleSearchMaxDepth && T >= 1 && T <= kNtupleMaxTuples && L >= 1 && L <= kNtupleMaxLen &&
           F <= kNtupleMaxFrac;
}

} // namespace

extern "C" {

// ntuple_search_root of n plain boards: action[n], value[n][4]; -1 for a depth or shape out of range
int ntuple_search_check_boards(const uint8_t *boards, uint64_t n, uint32_t depth, uint32_t T, uint32_t L, uint32_t F,
                               const uint8_t cells[8][6], const int32_t *weights, uint8_t *action, int64_t *value)
{
    if (!args_ok(depth, T, L, F))
        return -1;
    const NtupleShape sh = ntuple_shape(T, L, cells);
    with_shape(depth, T, [&](auto dc, auto tc) {
        for (uint64_t i = 0; i < n; ++i)
            action[i] = static_cast<uint8_t>(ntuple_search_root<decltype(dc)::value, decltype(tc)::value>(
                load_cells(boards + 16 * i), sh, F, weights, HostTables(), value + 4 * i));
    });
    return 0;
}

// The kernel's split on one thread: sum[n][4] = the sum over sub < K of ntuple_chance_partial(a_d, sub, K) (0 where d is
// illegal) -- for K = 1 the one-thread chance sum, before the division.
int ntuple_search_check_split(const uint8_t *boards, uint64_t n, uint32_t depth, uint32_t T, uint32_t L, uint32_t F,
                              const uint8_t cells[8][6], const int32_t *weights, uint32_t K, int64_t *sum)
{
    if (!args_ok(depth, T, L, F) || K < 1)
        return -1;
    const NtupleShape sh = ntuple_shape(T, L, cells);
    const HostTables tb;
    with_shape(depth, T, [&](auto dc, auto tc) {
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t d = 0; d < 4; ++d) {
                Board a = load_cells(boards + 16 * i);
                uint32_t gain;
                sum[4 * i + d] = 0;
                if (move_sel(a, tb.move_sel(d), gain))
                    for (uint32_t sub = 0; sub < K; ++sub)
                        sum[4 * i + d] += ntuple_chance_partial<decltype(dc)::value, decltype(tc)::value>(a, sub, K, sh, F, weights, tb);
            }
    });
    return 0;
}

int64_t ntuple_search_check_floor_div(int64_t a, int64_t b) { return floor_div(a, b); }

} // extern "C"
