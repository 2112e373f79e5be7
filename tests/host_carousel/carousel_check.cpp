// carousel_check.cpp -- the carousel code of g2048_device.h (the header the kernels are compiled from) built for the host
// (-DG2048_HOST_CHECK) on one thread: stage choice, sample index, ring slot and survival, the seen transition, the workgroup
// ranges, and a whole carousel step in the kernels' three passes (restart with entry marks and per-range counts, scan,
// scatter by rank) for any range size.  tests/test_carousel_host.py compares it with the pure-Python reference
// (tests/carousel_ref.py); the GPU tests compare the kernels with that reference too.  With -DCAROUSEL_CHECK_MAIN the file is
// a stand-alone program that drives the same code over random batches, for a sanitizer build.  Not part of the product.
#include "../host_common/ntuple_host.h"

#include <cstdio>
#include <vector>

namespace {

bool shape_ok(uint32_t S, const uint16_t *thr, uint32_t C)
{
    if (S < kCarouselMinStages || S > kNtupleMaxStages || C < 1 || C > kCarouselMaxCapacity || !thr)
        return false;
    for (uint32_t j = 0; j + 1 < S; ++j)
        if (thr[j] == 0 || (j > 0 && thr[j] <= thr[j - 1]))
            return false;
    return true;
}

} // namespace

extern "C" {

int carousel_check_stage(const uint8_t *records, uint64_t n, uint32_t S, const uint16_t *thr, uint8_t *out)
{
    if (!shape_ok(S, thr, 1))
        return -1;
    const CarouselStages cs = carousel_stages(S, thr);
    for (uint64_t i = 0; i < n; ++i)
        out[i] = static_cast<uint8_t>(carousel_stage(load_raw(records + 16 * i), cs));
    return 0;
}

uint32_t carousel_check_top(const uint64_t *count, uint32_t S) { return carousel_top_stage(count, S); }
uint32_t carousel_check_choice(uint32_t g, uint32_t e, uint32_t top) { return carousel_stage_choice(g, e, top); }
uint32_t carousel_check_fill(uint64_t count, uint32_t C) { return carousel_fill(count, C); }
uint32_t carousel_check_sample(uint32_t e, uint32_t g, uint32_t k, uint32_t fill, uint64_t seed)
{
    return carousel_sample(e, g, k, fill, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
}
uint32_t carousel_check_seen(uint32_t seen, uint32_t st) { return carousel_seen_next(seen, st); }
int carousel_check_is_entry(uint32_t seen) { return carousel_is_entry(seen) ? 1 : 0; }
// the slot of the entry of rank r among the m into a stage with `count` entries before the call, or -1 when it is dropped
int64_t carousel_check_slot(uint64_t count, uint32_t r, uint32_t m, uint32_t C)
{
    if (!carousel_survives(r, m, C))
        return -1;
    return carousel_slot(carousel_count_mod(count, C), r, C);
}
uint64_t carousel_check_range(uint64_t n, uint32_t block, uint32_t cap) { return carousel_range(n, block, cap); }

// One carousel step in the kernels' three passes over ranges of `per` boards (any per >= 1: the result must not depend on it)
int carousel_check_step(uint8_t *records, uint64_t n, uint64_t index_offset, const uint8_t *terminated, uint32_t S, const uint16_t *thr,
                        uint32_t C, uint64_t seed, uint8_t *pool, uint64_t *count, uint8_t *seen, uint32_t *episodes, uint64_t per)
{
    if (!shape_ok(S, thr, C) || n == 0 || per == 0 || index_offset + n > 0x100000000ull)
        return -1;
    const CarouselStages cs = carousel_stages(S, thr);
    const uint64_t groups = (n + per - 1) / per;
    std::vector<uint32_t> cnt(groups * kNtupleMaxStages, 0u), prefix(groups * kNtupleMaxStages, 0u);
    // restart: the pool and count are only read
    const uint32_t top = carousel_top_stage(count, S);
    for (uint64_t i = 0; i < n; ++i) {
        const Board rec = load_raw(records + 16 * i);
        if (terminated[i] != 0) {
            const uint32_t e = episodes[i];
            episodes[i] = e + 1u;
            const uint32_t g = static_cast<uint32_t>(index_offset + i);
            const uint32_t k = carousel_stage_choice(g, e, top);
            const uint64_t made = k > 0u ? count[k] : 0ull;
            if (made > 0ull) {
                const uint32_t j = carousel_sample(e, g, k, carousel_fill(made, C), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
                memcpy(records + 16 * i, pool + 16 * (static_cast<uint64_t>(k) * C + j), 16);
                seen[i] = static_cast<uint8_t>(k);
            } else {
                seen[i] = static_cast<uint8_t>(carousel_stage(rec, cs));
            }
        } else {
            const uint32_t st = carousel_stage(rec, cs);
            const uint32_t old = seen[i], next = carousel_seen_next(old, st);
            if (next != old) {
                seen[i] = static_cast<uint8_t>(next);
                if (next & kCarouselEntryBit)
                    ++cnt[(i / per) * kNtupleMaxStages + st];
            }
        }
    }
    // scan
    uint32_t total[kNtupleMaxStages] = {}, count_mod[kNtupleMaxStages] = {};
    for (uint32_t k = 1; k < S; ++k) {
        for (uint64_t w = 0; w < groups; ++w) {
            prefix[w * kNtupleMaxStages + k] = total[k];
            total[k] += cnt[w * kNtupleMaxStages + k];
        }
        count_mod[k] = carousel_count_mod(count[k], C);
        count[k] += total[k];
    }
    // scatter: the ranges in any order -- here the last first
    for (uint64_t w = groups; w-- > 0;) {
        uint32_t base[kNtupleMaxStages];
        for (uint32_t k = 0; k < kNtupleMaxStages; ++k)
            base[k] = prefix[w * kNtupleMaxStages + k];
        const uint64_t end = (w + 1) * per < n ? (w + 1) * per : n;
        for (uint64_t i = w * per; i < end; ++i) {
            if (!carousel_is_entry(seen[i]))
                continue;
            const uint32_t st = seen[i] & (kNtupleMaxStages - 1u);
            const uint32_t r = base[st]++;
            seen[i] = static_cast<uint8_t>(st);
            if (st >= 1u && st < S && carousel_survives(r, total[st], C))
                memcpy(pool + 16 * (static_cast<uint64_t>(st) * C + carousel_slot(count_mod[st], r, C)), records + 16 * i, 16);
        }
    }
    return 0;
}

} // extern "C"

#if defined(CAROUSEL_CHECK_MAIN)
// Random batches through carousel_check_step with exactly sized buffers, two range sizes that must agree.
int main()
{
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&x]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    const uint16_t thr[3] = {8, 16, 32};
    for (uint32_t round = 0; round < 40; ++round) {
        const uint64_t n = 1 + rnd() % 700;
        const uint32_t S = 2 + static_cast<uint32_t>(rnd() % 3), C = 1 + static_cast<uint32_t>(rnd() % 5);
        std::vector<uint8_t> pool_a(16ull * S * C, 0), seen_a(n, 0xff), rec_a(16 * n), term(n);
        std::vector<uint64_t> count_a(S, 0);
        std::vector<uint32_t> ep_a(n, round == 0 ? 0xfffffffeu : 0u);
        if (round == 1)
            count_a[1] = 0xffffffffffull; // beyond 2^32, not a multiple of C in general
        auto pool_b = pool_a, seen_b = seen_a, rec_b = rec_a;
        auto count_b = count_a;
        auto ep_b = ep_a;
        for (uint32_t step = 0; step < 12; ++step) {
            for (uint64_t i = 0; i < n; ++i) {
                term[i] = rnd() % 4 == 0;
                for (uint32_t j = 0; j < 16; ++j)
                    rec_a[16 * i + j] = rec_b[16 * i + j] = static_cast<uint8_t>((rnd() % 6) | (j >= 8 ? (rnd() & 0xe0) : 0));
            }
            const uint64_t offset = round % 2 ? 0x100000000ull - n : rnd() % 1000;
            if (carousel_check_step(rec_a.data(), n, offset, term.data(), S, thr, C, 7, pool_a.data(), count_a.data(), seen_a.data(),
                                    ep_a.data(), 256) ||
                carousel_check_step(rec_b.data(), n, offset, term.data(), S, thr, C, 7, pool_b.data(), count_b.data(), seen_b.data(),
                                    ep_b.data(), 1 + rnd() % 97)) {
                printf("carousel_check_step refused round %u\n", round);
                return 1;
            }
            if (rec_a != rec_b || pool_a != pool_b || count_a != count_b || seen_a != seen_b || ep_a != ep_b) {
                printf("range sizes disagree in round %u step %u\n", round, step);
                return 1;
            }
        }
    }
    printf("carousel driver ok\n");
    return 0;
}
#endif
