// Contour preparation (reference phoneme_to_articulation/__init__.py:57-118, phoneme_to_articulation/tail_clipper.py:7-128,
// scripts/calculate_normalization_statistics.py:73-75) on the device.
//
//   prepare_contours_kernel   one wave per (frame, articulator): the tail clipping of the tongue and the lips, the move into
//                             the upper-incisor frame ((p - u) + 0.3, two rounded operations) and the optional (x - mean) / std.
//                             The 50 points of a clipped contour sit on lanes 0..49.  Every clipping stage of the reference is
//                             "keep a subset of one half, then take F.interpolate(size=50) in nearest mode", i.e. output j is
//                             the kept point of rank floor(j n / 50): the kept set is a 64-bit __ballot mask, the source lane of
//                             an output is the position of the mask's s-th set bit (six popcount steps), the point comes by
//                             __shfl.  No LDS and no barrier: a wave past the last tile simply returns.
//                             The halves are [:25] and [25:] of the CURRENT list.  The tongue's and the upper lip's first stage
//                             leave the first 25 points untouched, so their second stage splits at the same place and the two
//                             stages are one mask; the lower lip resamples between its stages, so it takes two rounds.
//   column_stats_part_kernel  mean and centred sum of squares of CS_PART_ROWS rows of a (rows, cols) table, lane = column
//   column_stats_merge_kernel one wave per column merges the partitions by Chan's update in a fixed order
// The statistics are two-pass (mean, then centred sums) in fp64 after the fp32 load and rounded once at the end; the rows are
// partitioned by constants of this file (CS_PART_ROWS rows per partition, CS_WAVE_ROWS per wave, 64 partitions per lane
// stride), never by the launch geometry; no atomics: repeats are bit-identical.  pc_eval.hip's Chan updates are written into
// its kernels around states of their own (extrema, co-moments); the three-line merge of (count, mean, M2) is cs_merge here.
// Compiled without fused multiply-add contraction (build.py): every float32 result is the torch expression's, bit for bit.
#include "as_common.h"

#define CT_CLIP_N 50                                 // points per contour that the clipper is defined for
#define CT_HALF 25
#define CS_PART_ROWS AS_COLUMN_STATS_PART_ROWS       // rows per partition (workspace: 2 doubles per partition and column)
#define CS_WAVE_ROWS (CS_PART_ROWS / 4)              // rows per wave of a partition's workgroup

namespace {

// position of the s-th (0-based) set bit of mask; s < popcount(mask)
__device__ __forceinline__ int ct_select_bit(unsigned long long mask, int s) {
    int pos = 0;
#pragma unroll
    for (int b = 32; b > 0; b >>= 1) {
        const int c = __popcll((mask >> pos) & ((1ull << b) - 1ull));
        if (s >= c) { s -= c; pos += b; }
    }
    return pos;
}
// F.interpolate(size=50), nearest, of the n kept points (mask) of the wave's contour: lane j < 50 takes kept point (j n) / 50.
// Every lane of the wave executes the shuffles; n >= 1.
__device__ __forceinline__ void ct_resample(unsigned long long mask, int n, int lane, float& x, float& y) {
    const int s = lane < CT_CLIP_N ? (lane * n) / CT_CLIP_N : 0;
    const int src = ct_select_bit(mask, s);
    x = __shfl(x, src, 64);
    y = __shfl(y, src, 64);
}

// raw [F][A][N][2], refs [F][3][N][2] (lower incisor, upper incisor, epiglottis), kinds [A] or NULL, mean / std [A][2][N] or NULL.
// point_major == 0: out [F][A][2][N] in the incisor frame, ref_out [F][1][2][N] or NULL; point_major != 0: out [F][A][N][2], the
// clipped points as they are.  counts [F][A] or NULL.
__global__ __launch_bounds__(256) void prepare_contours_kernel(const float* __restrict__ raw, const float* __restrict__ refs,
                                                               const int32_t* __restrict__ kinds, int64_t tiles, int A, int N,
                                                               float thr0, float thr1, float thr2, float thr3,
                                                               const float* __restrict__ mean, const float* __restrict__ std,
                                                               int point_major, float* __restrict__ out,
                                                               float* __restrict__ ref_out, int32_t* __restrict__ counts) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile >= tiles) return;   // whole waves leave: nothing below synchronises across waves
    const int64_t f = tile / A;
    const int a = (int)(tile % A);
    const int kind = kinds ? kinds[a] : 0;
    const float2* p = reinterpret_cast<const float2*>(raw + tile * 2 * N);
    const float2* r_li = reinterpret_cast<const float2*>(refs + (f * 3 + 0) * 2 * N);
    const float2* r_ui = reinterpret_cast<const float2*>(refs + (f * 3 + 1) * 2 * N);
    const float2* r_ep = reinterpret_cast<const float2*>(refs + (f * 3 + 2) * 2 * N);
    const float2 u = r_ui[N - 1];   // the frame's origin: last point of the raw upper incisor
    float* o = out + tile * 2 * N;
    const float* mu = mean ? mean + (int64_t)a * 2 * N : nullptr;
    const float* sd = mean ? std + (int64_t)a * 2 * N : nullptr;

    if (ref_out && a == 0) {   // the frame's first tile carries the reference contour: never clipped, never normalised
        float* ro = ref_out + f * 2 * N;
        for (int i = lane; i < N; i += 64) {
            const float2 q = r_ui[i];
            ro[i] = __fadd_rn(__fsub_rn(q.x, u.x), 0.3f);
            ro[N + i] = __fadd_rn(__fsub_rn(q.y, u.y), 0.3f);
        }
    }

    int kept = N;
    if (kind == 0) {
        for (int i = lane; i < N; i += 64) {
            const float2 q = p[i];
            if (point_major) {
                o[2 * i] = q.x;
                o[2 * i + 1] = q.y;
                continue;
            }
            float x = __fadd_rn(__fsub_rn(q.x, u.x), 0.3f), y = __fadd_rn(__fsub_rn(q.y, u.y), 0.3f);
            if (mu) {
                x = __fdiv_rn(__fsub_rn(x, mu[i]), sd[i]);
                y = __fdiv_rn(__fsub_rn(y, mu[N + i]), sd[N + i]);
            }
            o[i] = x;
            o[N + i] = y;
        }
    } else {   // N == CT_CLIP_N (checked on the host): one point per lane
        const bool pt = lane < CT_CLIP_N;
        const bool first = lane < CT_HALF;
        float x = 0.f, y = 0.f;
        if (pt) {
            const float2 q = p[lane];
            x = q.x;
            y = q.y;
        }
        unsigned long long mask;
        if (kind == 3) {   // upper lip: above the incisor's last point minus a margin (margins at pixel scale, as the reference)
            const float lo = first ? __fsub_rn(u.y, thr3) : __fsub_rn(u.y, thr2);
            mask = __ballot(pt && y > lo);
        } else {
            const float li_max = as_wave_max(pt ? r_li[lane].y : -INFINITY);
            if (kind == 1) {   // tongue: front tail below the lower incisor's top, back tail below the epiglottis' bottom + margin
                const float ep_min = as_wave_min(pt ? r_ep[lane].y : INFINITY);
                const float hi = first ? __fadd_rn(ep_min, thr0) : li_max;
                mask = __ballot(pt && y < hi);
            } else {           // lower lip, stage 1: the second half against the incisor's top + margin, then resampled
                mask = __ballot(pt && (first || y < __fadd_rn(li_max, thr1)));
                ct_resample(mask, __popcll(mask), lane, x, y);   // >= 25 points
                mask = __ballot(pt && (!first || y < li_max));   // stage 2: the first half of the resampled list
            }
        }
        kept = __popcll(mask);
        if (kept > 0) {
            ct_resample(mask, kept, lane, x, y);
        } else {   // the reference raises inside F.interpolate: a NaN row and counts = 0 mark it
            x = y = __int_as_float(0x7fc00000);
        }
        if (pt) {
            if (point_major) {
                reinterpret_cast<float2*>(o)[lane] = make_float2(x, y);
            } else {
                if (kept > 0) {
                    x = __fadd_rn(__fsub_rn(x, u.x), 0.3f);
                    y = __fadd_rn(__fsub_rn(y, u.y), 0.3f);
                    if (mu) {
                        x = __fdiv_rn(__fsub_rn(x, mu[lane]), sd[lane]);
                        y = __fdiv_rn(__fsub_rn(y, mu[N + lane]), sd[N + lane]);
                    }
                }
                o[lane] = x;
                o[N + lane] = y;
            }
        }
    }
    if (counts && lane == 0) counts[tile] = kept;
}

// Chan's update of (n, mean, M2) by a batch (m, bmean, q); an empty batch changes nothing, an empty state takes the batch as it is
__device__ __forceinline__ void cs_merge(double& n, double& mean, double& M2, double m, double bmean, double q) {
    if (m == 0.0) return;
    if (n == 0.0) { n = m; mean = bmean; M2 = q; return; }
    const double nn = n + m, delta = bmean - mean;
    M2 = M2 + q + delta * delta * (n * m / nn);
    mean = mean + delta * (m / nn);
    n = nn;
}

// grid (partitions, column blocks of 64), 256 threads: wave w takes the rows [w CS_WAVE_ROWS, (w + 1) CS_WAVE_ROWS) of the
// partition, lane = column; the four waves' states are merged in wave order.  ws [partitions][2][cols] = mean | M2.
__global__ __launch_bounds__(256) void column_stats_part_kernel(const float* __restrict__ x, int64_t rows, int cols,
                                                                double* __restrict__ ws) {
    __shared__ double s_mean[4][64], s_m2[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t part = blockIdx.x;
    const int col = blockIdx.y * 64 + lane;
    const int64_t r0 = part * CS_PART_ROWS + (int64_t)wave * CS_WAVE_ROWS;
    const int64_t left = rows - r0;
    const int m = left <= 0 ? 0 : (left < CS_WAVE_ROWS ? (int)left : CS_WAVE_ROWS);
    double bmean = 0.0, q = 0.0;
    if (col < cols && m > 0) {
        const float* xp = x + r0 * cols + col;
        double s = 0.0;
        for (int r = 0; r < m; ++r) s += (double)xp[(int64_t)r * cols];
        bmean = s / (double)m;
        for (int r = 0; r < m; ++r) {
            const double d = (double)xp[(int64_t)r * cols] - bmean;
            q += d * d;
        }
    }
    s_mean[wave][lane] = bmean;
    s_m2[wave][lane] = q;
    __syncthreads();   // every wave of every block arrives: no wave returns before it
    if (wave != 0 || col >= cols) return;
    double n = 0.0, mean = 0.0, M2 = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int64_t lw = rows - (part * CS_PART_ROWS + (int64_t)w * CS_WAVE_ROWS);
        const double mw = lw <= 0 ? 0.0 : (lw < CS_WAVE_ROWS ? (double)lw : (double)CS_WAVE_ROWS);
        cs_merge(n, mean, M2, mw, s_mean[w][lane], s_m2[w][lane]);
    }
    ws[(part * 2 + 0) * cols + col] = mean;
    ws[(part * 2 + 1) * cols + col] = M2;
}

// one wave per column: lane l merges the partitions l, l + 64, ... in that order, then the xor butterfly merges the 64 lanes
__global__ __launch_bounds__(256) void column_stats_merge_kernel(const double* __restrict__ ws, int64_t rows, int cols,
                                                                 int64_t parts, float* __restrict__ mean_out,
                                                                 float* __restrict__ std_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + wave;
    if (col >= cols) return;
    double n = 0.0, mean = 0.0, M2 = 0.0;
    for (int64_t p = lane; p < parts; p += 64) {
        const int64_t left = rows - p * CS_PART_ROWS;
        const double m = left < CS_PART_ROWS ? (double)left : (double)CS_PART_ROWS;
        cs_merge(n, mean, M2, m, ws[(p * 2 + 0) * cols + col], ws[(p * 2 + 1) * cols + col]);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {   // the lower lane of a pair keeps (its state) + (the upper lane's): lane 0 ends with all
        const double on = __shfl_xor(n, o, 64), omean = __shfl_xor(mean, o, 64), oM2 = __shfl_xor(M2, o, 64);
        if ((lane & o) == 0) cs_merge(n, mean, M2, on, omean, oM2);
    }
    if (lane != 0) return;
    mean_out[col] = (float)mean;
    std_out[col] = (float)sqrt(M2 / (n - 1.0));   // unbiased; one row: 0 / 0 = NaN, like torch.std
}

}  // namespace

extern "C" int as_prepare_contours(const float* raw, const float* refs, const int32_t* kinds, int64_t F, int32_t A, int32_t N,
                                   float thr_tongue, float thr_lower_lip, float thr_upper_lip_front, float thr_upper_lip_back,
                                   const float* mean, const float* std, int32_t point_major, float* out, float* ref_out,
                                   int32_t* counts, void* stream) {
    AS_REQUIRE(raw && refs && out && F >= 1 && A >= 1 && N >= 1, AS_ERR_BAD_ARG, "as_prepare_contours: bad argument");
    AS_REQUIRE((mean == nullptr) == (std == nullptr), AS_ERR_BAD_ARG, "as_prepare_contours: mean and std come together");
    AS_REQUIRE(!point_major || (!mean && !ref_out), AS_ERR_BAD_ARG,
               "as_prepare_contours: the point-major output holds the clipped points only (no statistics, no reference output)");
    AS_REQUIRE(!kinds || N == CT_CLIP_N, AS_ERR_UNSUPPORTED, "as_prepare_contours: tail clipping is defined for %d points per contour, got %d",
               CT_CLIP_N, N);
    const int64_t tiles = F * A;
    AS_REQUIRE(tiles / 4 < 0x7fffffffLL, AS_ERR_UNSUPPORTED, "as_prepare_contours: %lld tiles exceed one grid", (long long)tiles);
    hipLaunchKernelGGL(prepare_contours_kernel, dim3(as_cdiv(tiles, 4)), dim3(256), 0, (hipStream_t)stream, raw, refs, kinds, tiles, A, N,
                       thr_tongue, thr_lower_lip, thr_upper_lip_front, thr_upper_lip_back, mean, std, point_major, out, ref_out, counts);
    AS_LAUNCH_CHECK("as_prepare_contours");
    return 0;
}

extern "C" int as_column_mean_std(const float* x, int64_t rows, int32_t cols, float* mean, float* std, double* ws, int64_t ws_doubles,
                                  void* stream) {
    AS_REQUIRE(x && mean && std && rows >= 1 && cols >= 1, AS_ERR_BAD_ARG, "as_column_mean_std: bad argument");
    const int64_t parts = (rows + CS_PART_ROWS - 1) / CS_PART_ROWS;
    AS_REQUIRE(parts < 0x7fffffffLL && as_cdiv(cols, 64) <= 65535, AS_ERR_UNSUPPORTED,
               "as_column_mean_std: %lld rows x %d columns exceed one grid", (long long)rows, cols);
    AS_REQUIRE(ws && ws_doubles >= 2 * parts * cols, AS_ERR_WORKSPACE, "as_column_mean_std: workspace of %lld doubles, %lld needed",
               (long long)ws_doubles, (long long)(2 * parts * cols));
    hipLaunchKernelGGL(column_stats_part_kernel, dim3((unsigned)parts, as_cdiv(cols, 64)), dim3(256), 0, (hipStream_t)stream, x, rows, cols,
                       ws);
    AS_LAUNCH_CHECK("as_column_mean_std (partitions)");
    hipLaunchKernelGGL(column_stats_merge_kernel, dim3(as_cdiv(cols, 4)), dim3(256), 0, (hipStream_t)stream, ws, rows, cols, parts, mean,
                       std);
    AS_LAUNCH_CHECK("as_column_mean_std (merge)");
    return 0;
}
