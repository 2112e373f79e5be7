// td_check.cpp -- ntuple_td_step of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK), two ways: inside the lane structure ntuple_td_step_kernel runs around it (whole blocks of lanes, the
// lanes past the end on board n - 1 and writing nothing, the episode counts per launch), and, as its check, the same step
// composed by hand of ntuple_root, ntuple_play_step, reset_record and ntuple_root.  All three shape types.
// tests/test_ntuple_td_host.py compares the two with each other and with tests/ntuple_play_ref.py.  Not part of the product.
#include "../host_common/ntuple_host.h"

#include <vector>

extern "C" {

// The outputs of one step of n boards, every array [n] (after and last_records [n][16]) and written for every board
// (last_records: where the episode ended); counts = {episodes, illegal_ends, gain_sum}, added to.
struct TdOut {
    uint8_t *action, *after;
    int64_t *after_value, *best_next;
    uint8_t *terminated;
    int64_t *delta;
    uint8_t *last_records;
    uint64_t *counts;
};

// The fused body in the kernel's lane structure, transaction t, records in place.  Returns the lanes that ran (a whole number
// of blocks), or -1.
int64_t td_check_fused(uint8_t *records, uint64_t n, uint64_t seed, uint64_t t, uint64_t board_offset, uint32_t max_exp, const Desc *d,
                       const int32_t *weights, const TdOut *out)
{
    if (!desc_ok(d, 2) || n == 0 || !out)
        return -1;
    const HostTables tb;
    const std::vector<uint8_t> loaded(records, records + 16 * n); // every lane loads before any lane stores
    const uint64_t lanes = (n + kBlockLanes - 1) / kBlockLanes * kBlockLanes;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        for (uint64_t i_raw = 0; i_raw < lanes; ++i_raw) {
            const bool valid = i_raw < n;
            const uint64_t i = valid ? i_raw : n - 1; // lane_of
            Board rec = load_raw(loaded.data() + 16 * i);
            const NtupleTdOut o =
                ntuple_td_step<T>(rec, t, static_cast<uint32_t>(board_offset + i), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                                  sh, d->F, weights, max_exp, tb, [&](const StepOut &st, const Board &terminal) {
                                      if (!(st.terminated && valid)) // record_episode_ends
                                          return;
                                      memcpy(out->last_records + 16 * i, terminal.r, 16);
                                      out->counts[0] += 1;
                                      out->counts[1] += st.legal ? 0 : 1;
                                  });
            if (!valid)
                continue;
            memcpy(records + 16 * i, rec.r, 16);
            out->action[i] = static_cast<uint8_t>(o.action);
            memcpy(out->after + 16 * i, o.after.r, 16);
            out->after_value[i] = o.after_value;
            out->best_next[i] = o.best_next;
            out->terminated[i] = o.step.terminated ? 1 : 0;
            out->delta[i] = o.delta;
            out->counts[2] += o.step.gain;
        }
    });
    return static_cast<int64_t>(lanes);
}

// The same step composed by hand of what g2048_ntuple_evaluate and g2048_ntuple_play are built from.  Returns n, -1, or -2 when
// ntuple_play_step did not play the first root's action.
int64_t td_check_composed(uint8_t *records, uint64_t n, uint64_t seed, uint64_t t, uint64_t board_offset, uint32_t max_exp, const Desc *d,
                          const int32_t *weights, const TdOut *out)
{
    if (!desc_ok(d, 2) || n == 0 || !out)
        return -1;
    const HostTables tb;
    int64_t rc = static_cast<int64_t>(n);
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        for (uint64_t i = 0; i < n; ++i) {
            Board rec = load_raw(records + 16 * i);
            const Board before = rec;
            const NtupleRoot r0 = ntuple_root<T>(record_cells(rec), sh, d->F, weights, tb);
            Words w;
            const StepOut o = ntuple_play_step<T>(rec, t, static_cast<uint32_t>(board_offset + i), static_cast<uint32_t>(seed),
                                                  static_cast<uint32_t>(seed >> 32), sh, d->F, weights, max_exp, tb, w);
            { // the move ntuple_play_step made is the first root's
                Board again = before;
                const StepOut o2 = play_record(again, r0.action, w, max_exp, tb);
                if (memcmp(again.r, rec.r, 16) != 0 || o2.terminated != o.terminated)
                    rc = -2;
            }
            if (o.terminated) {
                memcpy(out->last_records + 16 * i, rec.r, 16);
                out->counts[0] += 1;
                out->counts[1] += o.legal ? 0 : 1;
                reset_record(rec, o, w, tb);
            }
            const NtupleRoot r1 = ntuple_root<T>(record_cells(rec), sh, d->F, weights, tb);
            memcpy(records + 16 * i, rec.r, 16);
            out->action[i] = static_cast<uint8_t>(r0.action);
            memcpy(out->after + 16 * i, r0.after.r, 16);
            out->after_value[i] = r0.after_value;
            out->best_next[i] = r1.best;
            out->terminated[i] = o.terminated ? 1 : 0;
            out->delta[i] = static_cast<int64_t>((o.terminated ? 0ull : static_cast<uint64_t>(r1.best)) - static_cast<uint64_t>(r0.after_value));
            out->counts[2] += o.gain;
        }
    });
    return rc;
}

} // extern "C"
