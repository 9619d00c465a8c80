// Host-only planner of the resampler (csrc/resample.hip): the limits and the tile.  Plain C++, no HIP header, so that the checking
// program tests/resample_plan_check.cpp links it as it is.
#define AS_HOST_ONLY
#include "as_common.h"

// The first taps of a tile's outputs lie within floor((tile - 1) o / n) + 1 + spread samples of the tile's first one
// (floor(a + b) - floor(a) <= floor(b) + 1), and each output reads `band` samples from its first tap on.
extern "C" int64_t as_resample_span(int64_t tile, int32_t o, int32_t n, int32_t band, int32_t spread) {
    if (tile < 1 || o < 1 || n < 1 || band < 1 || spread < 0) return 0;
    return (tile - 1) * (int64_t)o / n + 2 + (int64_t)spread + band;
}

extern "C" int32_t as_resample_tile(int32_t o, int32_t n, int32_t band, int32_t spread) {
    if (o < 1 || o > AS_RESAMPLE_MAX_ROW || n < 1 || n > AS_RESAMPLE_MAX_PHASES || band < 1 || band > AS_RESAMPLE_MAX_BAND || spread < 0)
        return 0;
    for (int32_t tile = AS_RESAMPLE_MAX_TILE; tile >= 1; tile >>= 1)
        if (as_resample_span(tile, o, n, band, spread) <= AS_RESAMPLE_SPAN_FLOATS) return tile;
    return 0;
}
