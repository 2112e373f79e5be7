// log_check.cpp -- ntuple_play_log_step and ntuple_log_delta of g2048_device.h (the header the kernels are compiled from)
// built for the host (-DG2048_HOST_CHECK) and run in the lane structure ntuple_play_log_kernel and ntuple_log_delta_kernel run
// around them: whole blocks of lanes, the lanes past the end on board n - 1 and writing nothing; in play_log every lane's
// carry before its first move, the record kept over the M moves and stored once, the episode counts per launch; in log_delta
// one lane per board, the values behind the flags that ask for them.  All three shape types.
// tests/test_ntuple_log_host.py compares both with tests/ntuple_log_ref.py.  Not part of the product.
#include "../host_common/ntuple_host.h"

extern "C" {

// The log of n boards: depth M, after [M + 1][n][16], gain [M + 1][n], flag [M + 1][n]
struct HostLog {
    uint32_t depth;
    uint8_t *after;
    int64_t *gain;
    uint8_t *flag;
};

bool log_ok(const HostLog *lg) { return lg && lg->depth >= 1 && lg->depth <= kNtupleLogMaxDepth && lg->after && lg->gain && lg->flag; }

// One play_log launch: M moves from transaction t_first, records in place.  last_records [n][16]: the terminal record where an
// episode ended (the last one); counts = {episodes, illegal_ends, gain_sum}, added to.  Returns the lanes that ran, or -1.
int64_t log_check_play(uint8_t *records, uint64_t n, uint64_t seed, uint64_t t_first, uint64_t board_offset, uint32_t max_exp, const Desc *d,
                       const int32_t *weights, const HostLog *lg, uint8_t *last_records, uint64_t *counts)
{
    if (!desc_ok(d, 2) || n == 0 || !log_ok(lg) || !last_records || !counts)
        return -1;
    const HostTables tb;
    const uint64_t lanes = (n + kBlockLanes - 1) / kBlockLanes * kBlockLanes;
    const uint32_t M = lg->depth;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        for (uint64_t i_raw = 0; i_raw < lanes; ++i_raw) {
            const bool valid = i_raw < n;
            const uint64_t i = valid ? i_raw : n - 1; // lane_of
            Board rec = load_raw(records + 16 * i);
            // (a lane past the end works on board n - 1 as that board's own lane left it or will find it: it must write nothing.
            //  The record it loads may already be the stepped one here, where lanes run one after the other; it is dropped.)
            if (!valid)
                continue;
            const uint64_t last = static_cast<uint64_t>(M) * n;
            memcpy(lg->after + 16 * i, lg->after + 16 * (last + i), 16); // the carry
            lg->gain[i] = lg->gain[last + i];
            lg->flag[i] = lg->flag[last + i];
            uint64_t t = t_first;
            for (uint32_t m = 1; m <= M; ++m, ++t) {
                Words w;
                NtupleLogEntry e;
                const StepOut o = ntuple_play_log_step<T>(rec, t, static_cast<uint32_t>(board_offset + i), static_cast<uint32_t>(seed),
                                                          static_cast<uint32_t>(seed >> 32), sh, d->F, weights, max_exp, tb, w, e);
                const uint64_t slot = static_cast<uint64_t>(m) * n;
                memcpy(lg->after + 16 * (slot + i), e.after.r, 16);
                lg->gain[slot + i] = e.gain;
                lg->flag[slot + i] = static_cast<uint8_t>(e.flag);
                counts[2] += o.gain;
                if (o.terminated) { // record_episode_ends, then reset_record
                    memcpy(last_records + 16 * i, rec.r, 16);
                    counts[0] += 1;
                    counts[1] += o.legal ? 0 : 1;
                    reset_record(rec, o, w, tb);
                }
            }
            memcpy(records + 16 * i, rec.r, 16);
        }
    });
    return static_cast<int64_t>(lanes);
}

// One log_delta launch for slot m.  Returns the lanes that ran, -1 for a bad argument (m >= M included).  evaluations, when not
// NULL, += the ntuple_value calls made: what the flags skip is not evaluated.
int64_t log_check_delta(uint64_t n, const Desc *d, const int32_t *weights, const HostLog *lg, uint32_t m, int64_t *delta, uint64_t *evaluations)
{
    if (!desc_ok(d, 2) || n == 0 || !log_ok(lg) || m >= lg->depth || !delta)
        return -1;
    const uint64_t lanes = (n + kBlockLanes - 1) / kBlockLanes * kBlockLanes;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        for (uint64_t i = 0; i < lanes; ++i) {
            if (i >= n)
                continue;
            const uint64_t self = static_cast<uint64_t>(m) * n, next = self + n;
            const uint32_t f = lg->flag[self + i], f1 = lg->flag[next + i];
            int64_t v0 = 0, v1 = 0, gain1 = 0;
            if (ntuple_log_reads_self(f, f1)) {
                v0 = ntuple_value<T>(ntuple_pack(load_raw(lg->after + 16 * (self + i))), sh, weights);
                if (evaluations)
                    *evaluations += 1;
            }
            if (ntuple_log_reads_next(f, f1)) {
                gain1 = lg->gain[next + i];
                v1 = ntuple_value<T>(ntuple_pack(load_raw(lg->after + 16 * (next + i))), sh, weights);
                if (evaluations)
                    *evaluations += 1;
            }
            delta[i] = ntuple_log_delta(f, f1, gain1, v1, v0);
        }
    });
    return static_cast<int64_t>(lanes);
}

} // extern "C"
