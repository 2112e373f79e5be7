// ntuple_check.cpp -- the n-tuple network code of g2048_device.h (the header the kernels are compiled from) built for the
// host (-DG2048_HOST_CHECK), one board at a time on one thread.  tests/test_ntuple_host.py compares it with the pure-Python
// reference (tests/ntuple_ref.py); the GPU tests compare the kernels with that reference too.  Not part of the product.
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

// f(std::integral_constant<uint32_t, T>()) for the run-time T in 1..8; false for any other T
template <uint32_t T = 1, class F> bool with_tuples(uint32_t n_tuples, F &&f)
{
    if constexpr (T > kNtupleMaxTuples) {
        return false;
    } else {
        if (n_tuples == T) {
            f(std::integral_constant<uint32_t, T>());
            return true;
        }
        return with_tuples<T + 1>(n_tuples, f);
    }
}

bool shape_ok(uint32_t T, uint32_t L, uint32_t F) { return T >= 1 && T <= kNtupleMaxTuples && L >= 1 && L <= kNtupleMaxLen && F <= kNtupleMaxFrac; }

} // namespace

extern "C" {

// evaluate of n plain boards: value[n][4], action[n], best[n], after[n][16], after_value[n]; -1 for a shape out of range
int ntuple_check_evaluate(const uint8_t *boards, uint64_t n, uint32_t T, uint32_t L, uint32_t F, const uint8_t cells[8][6],
                          const int32_t *weights, int64_t *value, uint8_t *action, int64_t *best, uint8_t *after,
                          int64_t *after_value)
{
    if (!shape_ok(T, L, F))
        return -1;
    const NtupleShape sh = ntuple_shape(T, L, cells);
    with_tuples(T, [&](auto tc) {
        for (uint64_t i = 0; i < n; ++i) {
            const NtupleRoot r = ntuple_root<decltype(tc)::value>(load_cells(boards + 16 * i), sh, F, weights, HostTables());
            memcpy(value + 4 * i, r.q, sizeof(r.q));
            action[i] = static_cast<uint8_t>(r.action);
            best[i] = r.best;
            memcpy(after + 16 * i, r.after.r, 16);
            after_value[i] = r.after_value;
        }
    });
    return 0;
}

int ntuple_check_values(const uint8_t *boards, uint64_t n, uint32_t T, uint32_t L, const uint8_t cells[8][6], const int32_t *weights,
                        int64_t *v)
{
    if (!shape_ok(T, L, 0))
        return -1;
    const NtupleShape sh = ntuple_shape(T, L, cells);
    with_tuples(T, [&](auto tc) {
        for (uint64_t i = 0; i < n; ++i)
            v[i] = ntuple_value<decltype(tc)::value>(ntuple_pack(load_cells(boards + 16 * i)), sh, weights);
    });
    return 0;
}

// the update of n plain boards, in place on `weights`, board by board with a wrapping add
int ntuple_check_update(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t T, uint32_t L,
                        const uint8_t cells[8][6], int32_t *weights)
{
    if (!shape_ok(T, L, 0) || lr_shift > kNtupleMaxShift)
        return -1;
    const NtupleShape sh = ntuple_shape(T, L, cells);
    uint32_t *w = reinterpret_cast<uint32_t *>(weights);
    with_tuples(T, [&](auto tc) {
        for (uint64_t i = 0; i < n; ++i) {
            const int32_t step = ntuple_step(delta[i], lr_shift);
            if (step != 0)
                ntuple_update<decltype(tc)::value>(ntuple_pack(load_cells(boards + 16 * i)), sh, step,
                                                   [w](uint32_t off, int32_t st) { w[off] += static_cast<uint32_t>(st); });
        }
    });
    return 0;
}

int32_t ntuple_check_step(int64_t delta, uint32_t lr_shift) { return ntuple_step(delta, lr_shift); }

// the eight cell maps, out[8][16]: out[s][c] = ntuple_sym_cell(s, c)
void ntuple_check_sym_cells(uint8_t *out)
{
    for (uint32_t s = 0; s < 8; ++s)
        for (uint32_t c = 0; c < 16; ++c)
            out[16 * s + c] = static_cast<uint8_t>(ntuple_sym_cell(s, c));
}

} // extern "C"
