// Sample-rate conversion ahead of the log-mel (reference phoneme_recognition/datasets.py:124-126, F.resample) on the device: the
// polyphase windowed-sinc resampler of torchaudio's documentation, one launch from a padded batch of rows at `orig` to a padded
// batch at `new`.  The documentation's filter is dense, h [n phases][2 width + o taps], and its clamp leaves each phase a band of
// about 2 width + 2 non-zero taps; the host (features.Resample) builds the band alone, in float64, rounded to float32.
//
//   resample_kernel   one workgroup of 256 threads per (tile of `tile` consecutive outputs, row).  Output m = j n + i (phase i)
//                     reads the `band` input samples from floor(m o / n) + lead[i] on, lead[i] = first[i] - width - floor(i o / n)
//                     bounded by [lead_min, lead_max] over the phases, so a tile reads one contiguous span of
//                     floor((tile - 1) o / n) + 2 + (lead_max - lead_min) + band samples (as_resample_span):
//                       stage    the span into LDS, lanes along the samples (coalesced), zero outside [0, L): the zero padding
//                                of the formula and the guard against anything behind a row's samples in one test; int16
//                                samples become value / 32768 here (exact)
//                       sum      lane = output; adjacent lanes hold adjacent phases, so the coefficient of tap q, coef[q][i],
//                                is one coalesced read per wave served by the caches (the whole table is a few tens of KB and
//                                every workgroup reads all of it), and the samples come from LDS at a lane stride of o / n words
//                     The order of an output's sum depends on its phase and the band alone: four interleaved partial sums over
//                     q, then (s0 + s1) + (s2 + s3).  Neither the tile nor the batch enters: repeats, and a row alone or inside
//                     a batch, are bit-identical.
// The host chooses the tile (resample_plan.cpp) so that the span fits AS_RESAMPLE_SPAN_FLOATS floats of LDS.  An offset into the
// span is clamped to it, so a table that breaks the bounds it came with gives wrong values, never an access outside the span.
#include "as_common.h"

#define RS_THREADS 256

namespace {

__device__ __forceinline__ float rs_sample(const float* x, int64_t s) { return x[s]; }
__device__ __forceinline__ float rs_sample(const int16_t* x, int64_t s) { return (float)x[s] * (1.0f / 32768.0f); }

template <typename T>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const T* __restrict__ x, int64_t x_pitch, const int64_t* __restrict__ n_samples,
                                                              int o, int n, const float* __restrict__ coef, const int* __restrict__ first,
                                                              int band, int width, int lead_min, int tile, int span, float pad_value,
                                                              float* __restrict__ out, int64_t out_pitch, int64_t m_max,
                                                              int64_t* __restrict__ lengths_out) {
    extern __shared__ __align__(16) float rs_span[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t m0 = (int64_t)blockIdx.x * tile;
    int64_t L = n_samples[b];
    L = L < 0 ? 0 : (L > x_pitch ? x_pitch : L);
    int64_t M = ((int64_t)n * L + o - 1) / o;
    M = M > m_max ? m_max : M;
    if (lengths_out && blockIdx.x == 0 && tid == 0) lengths_out[b] = M;

    const int64_t lo = m0 * o / n + lead_min;   // the first sample of the tile's span
    if (m0 < M) {   // the same for every thread of the workgroup: a tile of padding alone skips to the store
        const T* row = x + (int64_t)b * x_pitch;
        for (int t = tid; t < span; t += RS_THREADS) {
            const int64_t s = lo + t;
            rs_span[t] = s >= 0 && s < L ? rs_sample(row, s) : 0.f;
        }
        __syncthreads();
    }

    const int64_t m_end = m0 + tile < m_max ? m0 + tile : m_max;
    float* y = out + (int64_t)b * out_pitch;
    for (int64_t m = m0 + tid; m < m_end; m += RS_THREADS) {
        float v = pad_value;
        if (m < M) {
            const int j = (int)m / n, i = (int)m - j * n;   // m < 2^30
            const int64_t at = (int64_t)j * o + ((int64_t)first[i] - width) - lo;   // in [0, span - band) for a table within its bounds
            const int off = (int)(at < 0 ? 0 : (at > span - band ? span - band : at));
            const float* c = coef + i;
            const float* xp = rs_span + off;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            int q = 0;
            for (; q + 3 < band; q += 4) {
                s0 = fmaf(c[q * n], xp[q], s0);
                s1 = fmaf(c[(q + 1) * n], xp[q + 1], s1);
                s2 = fmaf(c[(q + 2) * n], xp[q + 2], s2);
                s3 = fmaf(c[(q + 3) * n], xp[q + 3], s3);
            }
            for (; q < band; ++q) s0 = fmaf(c[q * n], xp[q], s0);
            v = (s0 + s1) + (s2 + s3);
        }
        y[m] = v;
    }
}

}  // namespace

extern "C" int as_resample_fwd(const void* x, int32_t x_int16, int64_t x_pitch, const int64_t* n_samples, int32_t B, int32_t o, int32_t n,
                               const float* coef, const int32_t* first, int32_t band, int32_t width, int32_t lead_min, int32_t lead_max,
                               float pad_value, float* out, int64_t out_pitch, int64_t m_max, int64_t* lengths_out, void* stream) {
    AS_REQUIRE(x && n_samples && coef && first && out && B >= 1 && x_pitch >= 1 && m_max >= 1 && out_pitch >= m_max && o >= 1 && n >= 1 &&
                   band >= 1 && width >= 0 && lead_max >= lead_min,
               AS_ERR_BAD_ARG, "as_resample_fwd: bad argument");
    AS_REQUIRE(n <= AS_RESAMPLE_MAX_PHASES && band <= AS_RESAMPLE_MAX_BAND, AS_ERR_UNSUPPORTED,
               "as_resample_fwd: %d phases (at most %d) or a band of %d taps (at most %d) not supported", n, AS_RESAMPLE_MAX_PHASES, band,
               AS_RESAMPLE_MAX_BAND);
    // offsets inside a row and the output index are 32-bit where the kernel divides: rows stay below 2^30 samples
    AS_REQUIRE(o <= AS_RESAMPLE_MAX_ROW && x_pitch <= AS_RESAMPLE_MAX_ROW && out_pitch <= AS_RESAMPLE_MAX_ROW, AS_ERR_UNSUPPORTED,
               "as_resample_fwd: rows of %lld -> %lld samples or a step of %d exceed the row limit of %d samples", (long long)x_pitch,
               (long long)out_pitch, o, AS_RESAMPLE_MAX_ROW);
    AS_REQUIRE((int64_t)lead_max - lead_min <= AS_RESAMPLE_SPAN_FLOATS && width <= AS_RESAMPLE_MAX_ROW && lead_min >= -AS_RESAMPLE_MAX_ROW &&
                   lead_max <= AS_RESAMPLE_MAX_ROW,
               AS_ERR_UNSUPPORTED, "as_resample_fwd: leads [%d, %d] around a width of %d not supported", lead_min, lead_max, width);
    const int spread = lead_max - lead_min;
    const int tile = as_resample_tile(o, n, band, spread);
    AS_REQUIRE(tile >= 1, AS_ERR_UNSUPPORTED,
               "as_resample_fwd: one output of %d -> %d with a band of %d taps reads more than the %d samples a workgroup stages", o, n, band,
               AS_RESAMPLE_SPAN_FLOATS);
    const int span = (int)as_resample_span(tile, o, n, band, spread);
    const int64_t tiles = (m_max + tile - 1) / tile;
    AS_REQUIRE(tiles < 0x7fffffffLL && B <= 65535, AS_ERR_UNSUPPORTED, "as_resample_fwd: %lld tiles x %d rows exceed one grid", (long long)tiles, B);
    const dim3 grid((unsigned)tiles, (unsigned)B);
    const size_t lds = (size_t)span * sizeof(float);
    if (x_int16)
        hipLaunchKernelGGL(resample_kernel<int16_t>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, (const int16_t*)x, x_pitch, n_samples, o, n,
                           coef, first, band, width, lead_min, tile, span, pad_value, out, out_pitch, m_max, lengths_out);
    else
        hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, (const float*)x, x_pitch, n_samples, o, n,
                           coef, first, band, width, lead_min, tile, span, pad_value, out, out_pitch, m_max, lengths_out);
    AS_LAUNCH_CHECK("as_resample_fwd");
    return 0;
}
