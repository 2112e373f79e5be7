// ntuple_trace_check.cpp -- the n-tuple trace code of g2048_device.h (the header the kernels are compiled from) built for
// the host (-DG2048_HOST_CHECK), one work item at a time on one thread, in the kernels' item order.
// tests/test_ntuple_trace_host.py compares it with the pure-Python reference (tests/ntuple_trace_ref.py); the GPU tests
// compare the kernels with that reference too.  Not part of the product.
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

// f(d_k, packed board) for every work item that has something to do, in item order
template <class F>
void for_items(uint64_t n, const int64_t *delta, uint32_t H, uint32_t lam, const uint8_t *hist, const uint8_t *len, uint32_t slot, F f)
{
    for (uint64_t item = 0; item < H * n; ++item) {
        uint32_t k, i;
        ntuple_trace_split(item, static_cast<uint32_t>(n), H, k, i);
        const int64_t dk = ntuple_trace_item(len[i], delta[i], k, H, lam);
        if (dk != 0)
            f(dk, ntuple_pack(load_cells(hist + (static_cast<uint64_t>(ntuple_trace_slot(slot, k, H)) * n + i) * 16)));
    }
}

} // namespace

extern "C" {

uint32_t ntuple_trace_check_decay(uint32_t lam, uint32_t k) { return ntuple_trace_decay(lam, k); }

// d_k of an unclamped delta: the clamp is part of what is checked
int64_t ntuple_trace_check_dk(int64_t delta, uint32_t lam, uint32_t k)
{
    return ntuple_trace_dk(ntuple_tc_delta(delta), ntuple_trace_decay(lam, k));
}

uint32_t ntuple_trace_check_push_len(uint32_t old, uint32_t H, uint32_t terminated) { return ntuple_trace_push_len(old, H, terminated != 0); }

uint32_t ntuple_trace_check_len(uint32_t len, uint32_t H) { return ntuple_trace_len(len, H); }

// (k << 32) | i of a work item
uint64_t ntuple_trace_check_split(uint64_t item, uint32_t n, uint32_t H)
{
    uint32_t k, i;
    ntuple_trace_split(item, n, H, k, i);
    return static_cast<uint64_t>(k) << 32 | i;
}

// push into `slot`, in place on hist / len, writing delta; -1 for H or slot out of range
int ntuple_trace_check_push(const uint8_t *after, const int64_t *after_value, const int64_t *best_next, const uint8_t *terminated,
                            uint64_t n, uint32_t H, uint8_t *hist, uint8_t *len, uint32_t slot, int64_t *delta)
{
    if (H < 1 || H > kNtupleTraceMax || slot >= H)
        return -1;
    for (uint64_t i = 0; i < n; ++i) {
        const bool term = terminated[i] != 0;
        memcpy(hist + (static_cast<uint64_t>(slot) * n + i) * 16, after + 16 * i, 16);
        delta[i] = ntuple_trace_delta(best_next[i], after_value[i], term);
        len[i] = static_cast<uint8_t>(ntuple_trace_push_len(len[i], H, term));
    }
    return 0;
}

// the trace update of n boards, in place on weights / err / mag.  mode 0: the TD form; mode 1..3: the TC form with
// phases = mode, phase W over every item, then phase A over every item.  -1 for an argument out of range.
int ntuple_trace_check_update(uint64_t n, const int64_t *delta, uint32_t lr_shift, uint32_t mode, uint32_t T, uint32_t L,
                              const uint8_t cells[8][6], int32_t *weights, int64_t *err, int64_t *mag, uint32_t H, uint32_t lam,
                              const uint8_t *hist, const uint8_t *len, uint32_t slot)
{
    if (T < 1 || T > kNtupleMaxTuples || L < 1 || L > kNtupleMaxLen || lr_shift > kNtupleMaxShift || mode > 3 || H < 1 ||
        H > kNtupleTraceMax || lam > kNtupleTcOne || slot >= H)
        return -1;
    const NtupleShape sh = ntuple_shape(T, L, cells);
    uint32_t *w = reinterpret_cast<uint32_t *>(weights);
    uint64_t *e = reinterpret_cast<uint64_t *>(err), *a = reinterpret_cast<uint64_t *>(mag);
    with_tuples(T, [&](auto tc) {
        constexpr uint32_t TT = decltype(tc)::value;
        auto add32 = [w](uint32_t off, int32_t st) { w[off] += static_cast<uint32_t>(st); };
        if (mode == 0)
            for_items(n, delta, H, lam, hist, len, slot, [&](int64_t dk, uint64_t packed) {
                const int32_t step = ntuple_step(dk, lr_shift);
                if (step != 0)
                    ntuple_update<TT>(packed, sh, step, add32);
            });
        if (mode & 1u)
            for_items(n, delta, H, lam, hist, len, slot,
                      [&](int64_t dk, uint64_t packed) { ntuple_tc_weights<TT>(packed, sh, dk, lr_shift, err, mag, add32); });
        if (mode & 2u)
            for_items(n, delta, H, lam, hist, len, slot, [&](int64_t dk, uint64_t packed) {
                ntuple_tc_accum<TT>(packed, sh, dk, [e, a](uint32_t off, int64_t dd, uint64_t m) {
                    e[off] += static_cast<uint64_t>(dd);
                    a[off] += m;
                });
            });
    });
    return 0;
}

} // extern "C"
