// mc_check.cpp -- TEST HARNESS ONLY: the Monte-Carlo rollout search of g2048_device.h compiled with g++
// (-DG2048_HOST_CHECK), one board at a time on one thread.  tests/test_mc_host.py compares it with the pure-Python
// reference (tests/mc_ref.py), the GPU tests compare the kernel with it, and tools/mc_probe.py plays whole games with it
// on the CPU.  Not part of the product.
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

bool any_legal(const Board &b)
{
    for (uint32_t d = 0; d < 4; ++d) {
        Board a = b;
        uint32_t g;
        if (move_sel(a, HostTables().move_sel(d), g))
            return true;
    }
    return false;
}

} // namespace

extern "C" {

// action[n], value[n][4], steps[n][4] of g2048_mc_search_plain; returns 0, or -1 for R or L outside their limits
int mc_check_boards(const uint8_t *boards, uint64_t n, uint32_t index_offset, uint32_t rollouts, uint32_t max_steps, uint64_t seed,
                    uint8_t *action, int64_t *value, int64_t *steps)
{
    if (rollouts < 1 || rollouts > kMcMaxRollouts || max_steps < 1 || max_steps > kMcMaxSteps)
        return -1;
    for (uint64_t i = 0; i < n; ++i)
        action[i] = (uint8_t)mc_root(load_cells(boards + 16 * i), index_offset + (uint32_t)i, rollouts, max_steps, (uint32_t)seed,
                                     (uint32_t)(seed >> 32), HostTables(), value + 4 * i, steps + 4 * i);
    return 0;
}

// the root sums through the kernel's lane split: K lanes per direction, lane sub sums the playouts sub, sub + K, ...
int mc_check_split(const uint8_t *boards, uint64_t n, uint32_t index_offset, uint32_t rollouts, uint32_t max_steps, uint64_t seed,
                   uint32_t K, int64_t *value, int64_t *steps)
{
    if (rollouts < 1 || rollouts > kMcMaxRollouts || max_steps < 1 || max_steps > kMcMaxSteps || K == 0)
        return -1;
    for (uint64_t i = 0; i < n; ++i) {
        const Board b = load_cells(boards + 16 * i);
        for (uint32_t d = 0; d < 4; ++d) {
            Board after = b;
            uint32_t g;
            value[4 * i + d] = steps[4 * i + d] = -1;
            if (!move_sel(after, HostTables().move_sel(d), g))
                continue;
            uint64_t total = 0, st = 0;
            for (uint32_t sub = K; sub-- > 0;) // the lanes in another order than mc_root's r = 0, 1, ...
                mc_partial(after, g, index_offset + (uint32_t)i, d, sub, K, rollouts, (uint32_t)seed, (uint32_t)(seed >> 32), max_steps,
                           HostTables(), total, st);
            value[4 * i + d] = (int64_t)total;
            steps[4 * i + d] = (int64_t)st;
        }
    }
    return 0;
}

// Whole games on the CPU: game k starts from fresh_board and is played to its end by the Monte-Carlo player
// (rollouts > 0; the search of move t is seeded seed + t + 1 and sees board index k) or, with rollouts == 0, by the
// uniform random policy under the engine's rule that an illegal move ends the episode.  The game's own spawns and the
// random policy's actions come from Philox blocks keyed by `seed` with counter word 3 = 0xffffffff.  scores[k] = the
// summed merge scores, moves[k] = the moves played; illegal_picks counts searched moves that were illegal while a legal
// one existed.  Returns that count.
uint64_t mc_check_play(uint64_t n_games, uint64_t seed, uint32_t rollouts, uint32_t max_steps, int64_t *scores, int64_t *moves)
{
    const HostTables tb;
    uint64_t illegal_picks = 0;
    for (uint64_t k = 0; k < n_games; ++k) {
        const Words w0 = philox4x32_10(0u, 0u, (uint32_t)k, 0xffffffffu, (uint32_t)seed, (uint32_t)(seed >> 32));
        Board b = fresh_board(w0.w[0], w0.w[1]);
        int64_t score = 0, t = 0;
        while (any_legal(b)) {
            const Words w = philox4x32_10((uint32_t)(t + 1), 0u, (uint32_t)k, 0xffffffffu, (uint32_t)seed, (uint32_t)(seed >> 32));
            uint32_t action = w.w[3] >> 30;
            if (rollouts > 0) {
                int64_t value[4], steps[4];
                const uint64_t s = seed + (uint64_t)t + 1u;
                action = mc_root(b, (uint32_t)k, rollouts, max_steps, (uint32_t)s, (uint32_t)(s >> 32), tb, value, steps);
            }
            uint32_t g;
            if (!move_sel(b, tb.move_sel(action), g)) {
                illegal_picks += rollouts > 0;
                break; // the engine's rule: an illegal move ends the episode
            }
            score += g;
            ++t;
            add_tile(b, w.w[0]);
        }
        scores[k] = score;
        moves[k] = t;
    }
    return illegal_picks;
}

} // extern "C"
