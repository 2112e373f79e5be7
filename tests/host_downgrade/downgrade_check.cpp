// downgrade_check.cpp -- downgrade_cells and ntuple_play_downgraded_step of g2048_device.h (the header the kernels are compiled
// from) built for the host (-DG2048_HOST_CHECK) on one thread: the rule on raw 16-byte boards, and the step inside the loop
// ntuple_play_downgraded_kernel runs around it (ntuple_play_check.cpp's loop, with the other step).  All three shape types.
// tests/test_downgrade_host.py compares both with tests/downgrade_ref.py.  Not part of the product.
#include "../host_common/ntuple_host.h"

extern "C" {

// out[i] = the translation of the 16 bytes boards[i] as they are (high bits and all), missing[i] = its k
int downgrade_check_rule(const uint8_t *boards, uint64_t n, uint32_t min_exp, uint32_t floor_exp, uint8_t *out, uint8_t *missing)
{
    if (min_exp < 1u || min_exp > 31u || floor_exp < kDowngradeMinFloor || floor_exp > 31u)
        return -1;
    const DowngradeRule rule{min_exp, floor_exp};
    for (uint64_t i = 0; i < n; ++i) {
        const Downgraded d = downgrade_cells(load_raw(boards + 16 * i), rule);
        memcpy(out + 16 * i, d.cells.r, 16);
        missing[i] = static_cast<uint8_t>(d.k);
    }
    return 0;
}

// ntuple_play_check_run (tests/host_ntuple_play) with ntuple_play_downgraded_step: the same arguments behind the rule's two,
// the same outputs; action[j][i] is the greedy action of the translated cells, computed here a second time
int downgrade_check_play(uint8_t *records, uint64_t n, uint64_t seed, uint64_t t_first, uint64_t board_offset, uint32_t k_steps,
                         uint32_t max_exp, const Desc *d, const int32_t *weights, uint32_t min_exp, uint32_t floor_exp,
                         uint32_t *games_left, uint8_t *terminated, uint8_t *action, uint8_t *last_records, uint64_t *episodes,
                         uint64_t *return_sum, uint64_t *gain_sum, uint64_t *hist, uint64_t *moves)
{
    if (!desc_ok(d, 2) || min_exp < 1u || min_exp > 31u || floor_exp < kDowngradeMinFloor || floor_exp > 31u)
        return -1;
    const HostTables tb;
    const DowngradeRule rule{min_exp, floor_exp};
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
                action[j * n + i] = static_cast<uint8_t>(ntuple_root<T>(downgrade_cells(rec, rule).cells, sh, d->F, weights, tb).action);
                Words w;
                const StepOut o = ntuple_play_downgraded_step<T>(rec, t, static_cast<uint32_t>(board_offset + i), static_cast<uint32_t>(seed),
                                                                 static_cast<uint32_t>(seed >> 32), sh, d->F, weights, max_exp, rule, tb, w);
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
