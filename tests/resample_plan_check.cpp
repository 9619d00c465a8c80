// Checking program of the resampler's host-only planner (artspeech_amd/csrc/resample_plan.cpp), built with the address and
// undefined-behaviour sanitizers by tests/test_resample_host.py and run on the CPU.  Over a sweep of ratios, bands and spreads:
// the tile is the largest power of two up to AS_RESAMPLE_MAX_TILE whose span fits the LDS budget, broken limits give 0, and --
// the property the kernel's LDS indexing rests on -- every output of every tile starts inside [0, span - band) of its tile's
// span, for leads anywhere inside their bounds.  Prints one summary line; any failure prints the case and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "artspeech_hip.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t bound) {   // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (uint32_t)(((state * 0x2545f4914f6cdd1dull) >> 33) % bound);
}

#define CHECK(cond, ...)            \
    do {                            \
        if (!(cond)) {              \
            printf(__VA_ARGS__);    \
            printf("\n");           \
            return 1;               \
        }                           \
    } while (0)

int main(void) {
    long plans = 0, refused = 0, outputs = 0;
    // limits
    CHECK(as_resample_tile(0, 1, 1, 0) == 0 && as_resample_tile(1, 0, 1, 0) == 0 && as_resample_tile(1, 1, 0, 0) == 0 &&
              as_resample_tile(1, 1, 1, -1) == 0,
          "a non-positive size was planned");
    CHECK(as_resample_tile(3, AS_RESAMPLE_MAX_PHASES + 1, 8, 1) == 0 && as_resample_tile(3, AS_RESAMPLE_MAX_PHASES, 8, 1) > 0, "phase limit");
    CHECK(as_resample_tile(3, 2, AS_RESAMPLE_MAX_BAND + 1, 1) == 0 && as_resample_tile(3, 2, AS_RESAMPLE_MAX_BAND, 1) > 0, "band limit");
    CHECK(as_resample_tile(AS_RESAMPLE_MAX_ROW, 1, 8, 0) == 1 && as_resample_tile(0x7fffffff, 1, 8, 0) == 0, "step limit");
    CHECK(as_resample_tile(3, 2, 8, 0x7fffffff) == 0 && as_resample_tile(3, 2, 8, AS_RESAMPLE_SPAN_FLOATS) == 0, "spread beyond the budget");
    CHECK(as_resample_span(0, 3, 2, 8, 1) == 0 && as_resample_span(1, 3, 2, 8, 1) == 11, "span of one output");
    CHECK(as_resample_tile(441, 160, 34, 1) == 1024 && as_resample_span(1024, 441, 160, 34, 1) == 2856, "44.1 -> 16 kHz");

    for (int it = 0; it < 20000; ++it) {
        const int32_t n = 1 + (int32_t)rnd(it % 4 == 0 ? AS_RESAMPLE_MAX_PHASES : 12);
        const int32_t o = 1 + (int32_t)rnd(it % 3 == 0 ? 20000 : 40);
        const int32_t band = 1 + (int32_t)rnd(AS_RESAMPLE_MAX_BAND);
        const int32_t spread = (int32_t)rnd(it % 5 == 0 ? 14000 : 4);
        const int32_t tile = as_resample_tile(o, n, band, spread);
        ++plans;
        if (tile == 0) {
            ++refused;
            CHECK(as_resample_span(1, o, n, band, spread) > AS_RESAMPLE_SPAN_FLOATS, "%d -> %d band %d spread %d refused, but one output fits", o, n,
                  band, spread);
            continue;
        }
        CHECK(tile >= 1 && tile <= AS_RESAMPLE_MAX_TILE && (tile & (tile - 1)) == 0, "%d -> %d: tile %d", o, n, tile);
        const int64_t span = as_resample_span(tile, o, n, band, spread);
        CHECK(span <= AS_RESAMPLE_SPAN_FLOATS && span > band, "%d -> %d: span %lld", o, n, (long long)span);
        CHECK(tile == AS_RESAMPLE_MAX_TILE || as_resample_span(2 * tile, o, n, band, spread) > AS_RESAMPLE_SPAN_FLOATS,
              "%d -> %d band %d spread %d: tile %d is not the largest that fits", o, n, band, spread, tile);
        if (it % 8) continue;
        // leads anywhere inside [lead_min, lead_min + spread], both ends taken: every output starts inside its tile's span
        const int32_t lead_min = -(int32_t)rnd(600);
        std::vector<int32_t> lead((size_t)n);
        for (int32_t i = 0; i < n; ++i) lead[(size_t)i] = lead_min + (int32_t)rnd((uint32_t)spread + 1);
        lead[rnd((uint32_t)n)] = lead_min + spread;
        lead[rnd((uint32_t)n)] = lead_min;
        std::vector<float> staged((size_t)span, 0.f);   // the tile's span as the kernel holds it: indexed below
        for (int t = 0; t < 3; ++t) {
            const int64_t m0 = (int64_t)rnd(1000000) * tile;
            const int64_t lo = m0 * o / n + lead_min;
            for (int64_t m = m0; m < m0 + tile; ++m, ++outputs) {
                const int64_t j = m / n, i = m - j * n;
                const int64_t at = j * o + i * o / n + lead[(size_t)i] - lo;
                CHECK(at >= 0 && at + band < span, "%d -> %d band %d spread %d tile %d: output %lld starts at %lld of a span of %lld", o, n, band,
                      spread, tile, (long long)m, (long long)at, (long long)span);
                staged[(size_t)at] += 1.f;
                staged[(size_t)(at + band - 1)] += 1.f;
            }
        }
    }
    printf("sweep: %ld plans, %ld refused, %ld outputs inside their spans\n", plans, refused, outputs);
    return 0;
}
