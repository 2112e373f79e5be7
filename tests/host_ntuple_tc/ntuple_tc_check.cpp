// ntuple_tc_check.cpp -- the temporal-coherence code of g2048_device.h (the header the kernels are compiled from) built for
// the host (-DG2048_HOST_CHECK), one board at a time on one thread.  tests/test_ntuple_tc_host.py compares it with the
// pure-Python reference (tests/ntuple_tc_ref.py); the GPU tests compare the kernels with that reference too.  Not part of
// the product.
#define G2048_HOST_CHECK 1
#include "../../gym-2048_amd/csrc/g2048_device.h"

#include <cstring>
#include <type_traits>

using namespace g2048;

namespace {

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

} // namespace

extern "C" {

uint32_t ntuple_tc_check_rate(int64_t err, uint64_t mag) { return ntuple_tc_rate(err, mag); }

// step of an unclamped delta: the clamp is part of what is checked
int32_t ntuple_tc_check_step(int64_t delta, uint32_t rate, uint32_t lr_shift)
{
    return ntuple_tc_step(ntuple_tc_delta(delta), rate, lr_shift);
}

// the update of n plain boards, in place on weights / err / mag: phase W over every board, then phase A over every board,
// with wrapping adds; -1 for a shape, shift or phases out of range
int ntuple_tc_check_update(const uint8_t *boards, uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t phases, uint32_t T,
                           uint32_t L, const uint8_t cells[8][6], int32_t *weights, int64_t *err, int64_t *mag)
{
    if (T < 1 || T > kNtupleMaxTuples || L < 1 || L > kNtupleMaxLen || lr_shift > kNtupleMaxShift || phases < 1 || phases > 3)
        return -1;
    const NtupleShape sh = ntuple_shape(T, L, cells);
    uint32_t *w = reinterpret_cast<uint32_t *>(weights);
    uint64_t *e = reinterpret_cast<uint64_t *>(err), *a = reinterpret_cast<uint64_t *>(mag);
    with_tuples(T, [&](auto tc) {
        for (uint64_t i = 0; (phases & 1u) && i < n; ++i) {
            const int64_t d = ntuple_tc_delta(delta[i]);
            if (d != 0)
                ntuple_tc_weights<decltype(tc)::value>(ntuple_pack(load_cells(boards + 16 * i)), sh, d, lr_shift, err, mag,
                                                       [w](uint32_t off, int32_t st) { w[off] += static_cast<uint32_t>(st); });
        }
        for (uint64_t i = 0; (phases & 2u) && i < n; ++i) {
            const int64_t d = ntuple_tc_delta(delta[i]);
            if (d != 0)
                ntuple_tc_accum<decltype(tc)::value>(ntuple_pack(load_cells(boards + 16 * i)), sh, d,
                                                     [e, a](uint32_t off, int64_t dd, uint64_t m) {
                                                         e[off] += static_cast<uint64_t>(dd);
                                                         a[off] += m;
                                                     });
        }
    });
    return 0;
}

} // extern "C"
