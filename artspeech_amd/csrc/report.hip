// Per-sentence correlation of the result tables (reference report_phoneme_to_articulation.py:256-285: groupby("sentence")
// [[target, pred]].corr() per tract variable, then mean / std / min / max of the sentences' coefficients) on the device.
//
//   segment_corr_kernel      one wave per (segment, column): Pearson's r of a[rows of the segment][k] and b[..][k], each value
//                            (double)x * scale (the table in mm, rounded once like the reference's column product)
//   segment_summary_kernel   one wave per column: count / mean / std (n - 1) / min / max of the finite coefficients
// Both reduce in two passes (mean, then centred sums), fp64 after the fp32 load.  Lane l takes the elements l, l + 64, ... of
// its segment and the butterfly adds the 64 partials in one order: nothing depends on the launch geometry, no atomics,
// repeats are bit-identical.  Compiled without fused multiply-add contraction (build.py): x * scale is rounded before the
// mean is taken from it.
#include "as_common.h"

namespace {

// A column whose values are all the same float has no correlation (pandas: NaN); the centred sums of such a column are
// rounding noise whenever its mean is not representable (x * scale summed n times), so the case is decided on the bits.
__global__ __launch_bounds__(256) void segment_corr_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t rows,
                                                           int K, double scale, const int64_t* __restrict__ seg_first,
                                                           int64_t pairs, double* __restrict__ corr) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + wave;
    if (pair >= pairs) return;   // whole waves leave: no barrier below
    const int64_t s = pair / K;
    const int k = (int)(pair % K);
    int64_t r0 = seg_first[s], r1 = seg_first[s + 1];
    r0 = r0 < 0 ? 0 : r0;         // a segment never reaches outside the table
    r1 = r1 > rows ? rows : r1;
    const int64_t n = r1 - r0;
    if (n < 2) {
        if (lane == 0) corr[pair] = NAN;
        return;
    }
    const unsigned a0 = __float_as_uint(a[r0 * K + k]), b0 = __float_as_uint(b[r0 * K + k]);
    double sa = 0.0, sb = 0.0;
    int differs_a = 0, differs_b = 0;
    for (int64_t r = r0 + lane; r < r1; r += 64) {
        const float xa = a[r * K + k], xb = b[r * K + k];
        differs_a |= __float_as_uint(xa) != a0;
        differs_b |= __float_as_uint(xb) != b0;
        sa += (double)xa * scale;
        sb += (double)xb * scale;
    }
    sa = as_wave_sum_d(sa);
    sb = as_wave_sum_d(sb);
    const bool constant = !__any(differs_a) || !__any(differs_b);
    const double ma = sa / (double)n, mb = sb / (double)n;
    double qab = 0.0, qaa = 0.0, qbb = 0.0;
    for (int64_t r = r0 + lane; r < r1; r += 64) {
        const double da = (double)a[r * K + k] * scale - ma, db = (double)b[r * K + k] * scale - mb;
        qab = fma(da, db, qab);
        qaa = fma(da, da, qaa);
        qbb = fma(db, db, qbb);
    }
    qab = as_wave_sum_d(qab);
    qaa = as_wave_sum_d(qaa);
    qbb = as_wave_sum_d(qbb);
    if (lane == 0) corr[pair] = constant ? (double)NAN : qab / sqrt(qaa * qbb);
}

// summary [5][K]: count | mean | std | min | max over the finite corr[s][k], s < S.
__global__ __launch_bounds__(256) void segment_summary_kernel(const double* __restrict__ corr, int S, int K,
                                                              double* __restrict__ summary) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + wave;
    if (k >= K) return;
    double s = 0.0, m = 0.0;
    for (int i = lane; i < S; i += 64) {
        const double c = corr[(int64_t)i * K + k];
        if (isfinite(c)) { s += c; m += 1.0; }
    }
    s = as_wave_sum_d(s);
    m = as_wave_sum_d(m);
    const double mean = s / m;   // 0 / 0 = NaN without a finite coefficient
    double q = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int i = lane; i < S; i += 64) {
        const double c = corr[(int64_t)i * K + k];
        if (isfinite(c)) {
            const double d = c - mean;
            q = fma(d, d, q);
            mn = fmin(mn, c);
            mx = fmax(mx, c);
        }
    }
    q = as_wave_sum_d(q);
    mn = as_wave_min_d(mn);
    mx = as_wave_max_d(mx);
    if (lane != 0) return;
    summary[k] = m;
    summary[K + k] = mean;
    summary[2 * K + k] = m < 2.0 ? (double)NAN : sqrt(q / (m - 1.0));
    summary[3 * K + k] = m == 0.0 ? (double)NAN : mn;
    summary[4 * K + k] = m == 0.0 ? (double)NAN : mx;
}

}  // namespace

extern "C" int as_segment_corr(const float* a, const float* b, int64_t rows, int32_t K, double scale, const int64_t* seg_first,
                               int32_t S, double* corr, double* summary, void* stream) {
    AS_REQUIRE(K >= 1 && S >= 0 && rows >= 0, AS_ERR_BAD_ARG, "as_segment_corr: K %d, S %d, rows %lld", K, S, (long long)rows);
    AS_REQUIRE(summary && (S == 0 || (seg_first && corr)) && (rows == 0 || (a && b)), AS_ERR_BAD_ARG,
               "as_segment_corr: null argument");
    const int64_t pairs = (int64_t)S * K;
    AS_REQUIRE(pairs / 4 < 0x7fffffffLL, AS_ERR_UNSUPPORTED, "as_segment_corr: %lld (segment, column) pairs exceed one grid",
               (long long)pairs);
    if (pairs > 0) {
        hipLaunchKernelGGL(segment_corr_kernel, dim3(as_cdiv(pairs, 4)), dim3(256), 0, (hipStream_t)stream, a, b, rows, K, scale,
                           seg_first, pairs, corr);
        AS_LAUNCH_CHECK("as_segment_corr (coefficients)");
    }
    hipLaunchKernelGGL(segment_summary_kernel, dim3(as_cdiv(K, 4)), dim3(256), 0, (hipStream_t)stream, corr, S, K, summary);
    AS_LAUNCH_CHECK("as_segment_corr (summary)");
    return 0;
}
