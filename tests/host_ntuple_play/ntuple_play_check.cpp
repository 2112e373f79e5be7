// ntuple_play_check.cpp -- ntuple_play_step of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK) on one thread, inside the loop ntuple_play_kernel runs around it: the budget test, the step, the
// episode end (terminal record, histogram), reset_record, the budget's decrement.  All three shape types.
// tests/test_ntuple_play_host.py compares it with tests/ntuple_play_ref.py.  Not part of the product.
#include "../host_common/ntuple_host.h"

extern "C" {

// k_steps of the fused player on n records, in place, transactions t_first .. t_first + k_steps - 1.  games_left may be NULL.
// Out: terminated[k_steps][n], action[k_steps][n] (0xff where the board sat the step out), last_records[n][16] (written
// where an episode ended), episodes[n], return_sum (the scores of the terminal records), gain_sum, hist[32], moves.
int ntuple_play_check_run(uint8_t *records, uint64_t n, uint64_t seed, uint64_t t_first, uint64_t board_offset, uint32_t k_steps,
                          uint32_t max_exp, const Desc *d, const int32_t *weights, uint32_t *games_left, uint8_t *terminated,
                          uint8_t *action, uint8_t *last_records, uint64_t *episodes, uint64_t *return_sum, uint64_t *gain_sum,
                          uint64_t *hist, uint64_t *moves)
{
    if (!desc_ok(d, 2))
        return -1;
    const HostTables tb;
    with_tuples(d, [&](auto tc, const auto &sh) {
        constexpr uint32_t T = decltype(tc)::value;
        for (uint64_t i = 0; i < n; ++i) {
            Board rec = load_raw(records + 16 * i);
            uint32_t left = games_left ? games_left[i] : 1u;
            uint64_t t = t_first;
            for (uint32_t j = 0; j < k_steps; ++j, ++t) {
                terminated[j * n + i] = 0;
                action[j * n + i] = 0xffu;
                if (left == 0u)
                    continue;
                action[j * n + i] = static_cast<uint8_t>(ntuple_root<T>(record_cells(rec), sh, d->F, weights, tb).action);
                Words w;
                const StepOut o = ntuple_play_step<T>(rec, t, static_cast<uint32_t>(board_offset + i), static_cast<uint32_t>(seed),
                                                      static_cast<uint32_t>(seed >> 32), sh, d->F, weights, max_exp, tb, w);
                *moves += 1;
                *gain_sum += o.gain;
                if (!o.terminated)
                    continue;
                terminated[j * n + i] = 1;
                memcpy(last_records + 16 * i, rec.r, 16);
                episodes[i] += 1;
                *return_sum += record_score(rec);
                hist[highest(record_cells(rec))] += 1;
                reset_record(rec, o, w, tb);
                if (games_left)
                    left -= 1u;
            }
            memcpy(records + 16 * i, rec.r, 16);
            if (games_left)
                games_left[i] = left;
        }
    });
    return 0;
}

} // extern "C"
