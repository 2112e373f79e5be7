// restart_check.cpp -- restart_board of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK) and run in the lane structure restart_step_kernel runs around it: `groups` workgroups of kBlockLanes
// lanes striding over the boards, pos read by every lane, start and restarts only where the episode ended, each written back
// only where the kernel writes it.  tests/test_restart_host.py compares it with tests/restart_ref.py.
// With -DRESTART_CHECK_MAIN the file is a stand-alone program: main() runs the same function over random states of every
// stride and capacity edge against a model written out in main's own words, for a run under -fsanitize=address,undefined.
// Not part of the product.
#include "../host_common/ntuple_host.h"

extern "C" {

struct HostRestart {
    uint32_t stride_log2, capacity, min_span, max_restarts;
    uint8_t *snap;                    // [C][n][16]
    uint32_t *pos, *start, *restarts; // [n]
};

bool restart_ok(const HostRestart *r)
{
    return r && r->stride_log2 <= kRestartMaxStrideLog2 && r->capacity >= 1 && r->capacity <= kRestartMaxCapacity &&
           r->min_span >= kRestartMinSpan && r->min_span <= kRestartMaxSpan && r->max_restarts >= 1 && r->snap && r->pos && r->start &&
           r->restarts;
}

// One restart step on n records in place, as a launch of `groups` workgroups.  Returns the loop trips of lane 0 of workgroup 0
// (how often the grid-stride loop ran), or -1 for a bad argument.
int64_t restart_check_step(uint8_t *records, uint64_t n, const uint8_t *terminated, const HostRestart *r, uint32_t groups)
{
    if (!restart_ok(r) || !records || !terminated || n == 0 || n > 0xffffff00ull || groups == 0)
        return -1;
    const RestartRule rule{r->stride_log2, r->capacity, r->min_span, r->max_restarts};
    uint4 *snap = reinterpret_cast<uint4 *>(r->snap);
    const uint64_t stride = static_cast<uint64_t>(groups) * kBlockLanes;
    int64_t trips = 0;
    for (uint64_t lane = 0; lane < stride; ++lane) {
        for (uint64_t g = lane; g < n; g += stride) {
            const uint32_t i = static_cast<uint32_t>(g);
            const bool ended = terminated[i] != 0;
            RestartBoard b{r->pos[i], 0u, 0u};
            const uint32_t pos = b.pos;
            if (ended) {
                b.start = r->start[i];
                b.restarts = r->restarts[i];
            }
            restart_board(RestartRecordStored{reinterpret_cast<uint4 *>(records), i}, ended, rule, snap, static_cast<uint32_t>(n), i, b);
            if (b.pos != pos)
                r->pos[i] = b.pos;
            if (ended) {
                r->start[i] = b.start;
                r->restarts[i] = b.restarts;
            }
            trips += lane == 0;
        }
    }
    return trips;
}

} // extern "C"

#if defined(RESTART_CHECK_MAIN)
#include <cstdio>
#include <vector>

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return static_cast<uint32_t>(g_rng >> 16);
}

struct Batch {
    uint32_t n;
    std::vector<uint8_t> records, terminated, snap;
    std::vector<uint32_t> pos, start, restarts;
};

// the rule of include/g2048.h in 64-bit arithmetic, one board after the other
void model_step(Batch &b, uint32_t k, uint32_t C, uint32_t min_span, uint32_t max_restarts)
{
    const uint64_t s = 1ull << k;
    for (uint32_t i = 0; i < b.n; ++i) {
        if (!b.terminated[i]) {
            if (b.pos[i] == 0xffffffffu)
                continue;
            const uint64_t p = static_cast<uint64_t>(b.pos[i]) + 1;
            b.pos[i] = static_cast<uint32_t>(p);
            if (p % s == 0 && p / s >= 1 && p / s <= C)
                memcpy(&b.snap[((p / s - 1) * b.n + i) * 16], &b.records[16ull * i], 16);
            continue;
        }
        const uint64_t S = b.start[i], R = (b.pos[i] - b.start[i]) & 0xffffffffull, m = (S + R / 2) & 0xffffffffull;
        const uint64_t q = m / s < C ? m / s : C, S1 = q * s;
        if (R >= min_span && b.restarts[i] < max_restarts && q >= 1 && S1 > S) {
            memcpy(&b.records[16ull * i], &b.snap[((q - 1) * b.n + i) * 16], 16);
            b.start[i] = b.pos[i] = static_cast<uint32_t>(S1);
            b.restarts[i] += 1;
        } else {
            b.start[i] = b.pos[i] = b.restarts[i] = 0;
        }
    }
}

} // namespace

int main()
{
    const uint32_t ks[] = {0, 1, 4, 16}, caps[] = {1, 2, 5, 64}, ns[] = {1, 63, 197, 700};
    uint64_t checked = 0, restarted = 0;
    for (uint32_t k : ks)
        for (uint32_t C : caps)
            for (uint32_t n : ns) {
                const uint32_t s = 1u << k, min_span = 2 + rnd() % 7, max_restarts = 1 + rnd() % 3;
                Batch a{n, {}, {}, {}, {}, {}, {}};
                a.records.resize(16ull * n);
                a.terminated.resize(n);
                a.snap.resize(16ull * C * n);
                a.pos.resize(n);
                a.start.resize(n);
                a.restarts.resize(n);
                for (auto &x : a.records)
                    x = static_cast<uint8_t>(rnd());
                for (auto &x : a.snap)
                    x = static_cast<uint8_t>(rnd());
                for (uint32_t i = 0; i < n; ++i) { // positions around the stride multiples, the last slot and the end of the range
                    const uint32_t q = rnd() % (C + 3);
                    a.start[i] = (rnd() % (C + 1)) * s;
                    a.pos[i] = rnd() % 16 == 0 ? 0xffffffffu - rnd() % 2 : q * s + rnd() % 3 - 1u + (q == 0);
                    if (a.pos[i] < a.start[i] && rnd() % 4)
                        a.pos[i] = a.start[i] + rnd() % (4 * s);
                    a.restarts[i] = rnd() % 4;
                }
                Batch b = a;
                for (uint32_t step = 0; step < 6; ++step) {
                    for (uint32_t i = 0; i < n; ++i)
                        a.terminated[i] = b.terminated[i] = rnd() % 3 == 0;
                    HostRestart r{k, C, min_span, max_restarts, a.snap.data(), a.pos.data(), a.start.data(), a.restarts.data()};
                    const int64_t trips = restart_check_step(a.records.data(), n, a.terminated.data(), &r, 1 + step % 2);
                    if (trips != static_cast<int64_t>((n + (1 + step % 2) * kBlockLanes - 1) / ((1 + step % 2) * kBlockLanes))) {
                        printf("restart_check: %lld trips at n=%u\n", static_cast<long long>(trips), n);
                        return 1;
                    }
                    std::vector<uint32_t> had = b.restarts;
                    model_step(b, k, C, min_span, max_restarts);
                    for (uint32_t i = 0; i < n; ++i)
                        restarted += b.restarts[i] == had[i] + 1;
                    if (a.records != b.records || a.snap != b.snap || a.pos != b.pos || a.start != b.start || a.restarts != b.restarts) {
                        printf("restart_check: mismatch at k=%u C=%u n=%u step=%u\n", k, C, n, step);
                        return 1;
                    }
                    checked += n;
                }
            }
    if (restarted < 100) {
        printf("restart_check: only %llu restarts\n", static_cast<unsigned long long>(restarted));
        return 1;
    }
    printf("restart_check ok: %llu board-steps, %llu restarts\n", static_cast<unsigned long long>(checked),
           static_cast<unsigned long long>(restarted));
    return 0;
}
#endif
