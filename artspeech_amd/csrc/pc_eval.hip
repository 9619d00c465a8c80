// Evaluation of the principal-components method (reference phoneme_to_articulation/principal_components/evaluation.py and
// test_principal_components_autoencoder.py:92-208) on the device.
//
//   pc_shapes_eval_kernel   one wave per (row, articulator) tile: denormalise prediction and target (x * std + mean, each
//                           operation rounded: the dumped contours equal the torch expression bit for bit), write both in the
//                           layout save_outputs / tract_variables_batched take (reference contour copied in at ref_idx), and
//                           the MeanP2CPDistance in mm of the pair from the same staged points (direct differences, like
//                           metrics.hip's p2cp_kernel)
//   pc_eval_errors_kernel   count / mean / M2 / min / max of the per-frame errors of a split, one wave per articulator
//   pc_eval_latents_kernel  count / mean / centred co-moments of the latents of a split, one workgroup
// Both accumulators reduce a batch in two passes (mean, then centred sums) and merge it into a device-resident fp64 state by
// Chan's update, the rule pca.hip's chain applies to its mean and variance (there it is woven into the chain kernel's step; the
// states differ -- variance per feature there, a co-moment matrix and extrema here -- so the few lines are restated).  Every
// sum is partitioned by constants of this file (64 lanes, 4 row partitions), never by the launch geometry, and added in a
// fixed order: no atomics, bit-identical repeats.  Compiled without fused multiply-add contraction (build.py).
#include "as_common.h"
#include "as_device.h"

#define PCE_MAX_N 128     // points per contour: 2 N <= 256, the width limit of the fused MLP kernel
#define PCE_MAX_L 64      // latent size: k_max of the PCA
#define PCE_CHUNK 32      // rows of centred latents staged per step
#define PCE_PAIRS 16      // co-moments per thread: PCE_MAX_L^2 / 256

namespace {

__device__ __forceinline__ bool pce_valid(const int32_t* __restrict__ lengths, int T, int64_t r) {
    return !lengths || (int)(r % T) < lengths[r / T];
}

__global__ __launch_bounds__(256) void pc_shapes_eval_kernel(const float* __restrict__ shapes, const float* __restrict__ targets,
                                                             const float* __restrict__ mean, const float* __restrict__ std,
                                                             const int32_t* __restrict__ lengths, int T,
                                                             const float* __restrict__ reference, int ref_idx, int64_t tiles, int A,
                                                             int N, float to_mm, float* __restrict__ pred_out,
                                                             float* __restrict__ tgt_out, float* __restrict__ p2cp_mm) {
    __shared__ __attribute__((aligned(16))) float smem[4][4 * PCE_MAX_N];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const int N4 = (N + 3) & ~3;   // padded with +inf: a padding point is never a minimum
    float* px = smem[wave];
    float* py = px + N4;
    float* tx = py + N4;
    float* ty = tx + N4;
    const bool live = tile < tiles;
    bool valid = false;
    if (live) {
        const int64_t row = tile / A;
        const int a = (int)(tile % A);
        valid = pce_valid(lengths, T, row);
        const int C = A + (ref_idx >= 0 ? 1 : 0), co = a + ((ref_idx >= 0 && a >= ref_idx) ? 1 : 0);
        const float* s = shapes + tile * 2 * N;
        const float* t = targets + tile * 2 * N;
        const float* mu = mean + (int64_t)a * 2 * N;
        const float* sd = std + (int64_t)a * 2 * N;
        float* po = pred_out ? pred_out + (row * C + co) * 2 * N : nullptr;
        float* to = tgt_out ? tgt_out + (row * C + co) * 2 * N : nullptr;
        for (int i = lane; i < N4; i += 64) {
            float vpx = INFINITY, vpy = INFINITY, vtx = INFINITY, vty = INFINITY;
            if (i < N) {
                if (valid) {
                    vpx = __fadd_rn(__fmul_rn(s[i], sd[i]), mu[i]);
                    vpy = __fadd_rn(__fmul_rn(s[N + i], sd[N + i]), mu[N + i]);
                    vtx = __fadd_rn(__fmul_rn(t[i], sd[i]), mu[i]);
                    vty = __fadd_rn(__fmul_rn(t[N + i], sd[N + i]), mu[N + i]);
                }
                if (po) { po[i] = valid ? vpx : 0.f; po[N + i] = valid ? vpy : 0.f; }
                if (to) { to[i] = valid ? vtx : 0.f; to[N + i] = valid ? vty : 0.f; }
            }
            px[i] = vpx; py[i] = vpy; tx[i] = vtx; ty[i] = vty;
        }
        if (a == 0 && ref_idx >= 0) {   // the row's first tile carries the reference contour into both outputs
            const float* ref = reference + row * 2 * N;
            for (int i = lane; i < 2 * N; i += 64) {
                const float v = valid ? ref[i] : 0.f;
                if (pred_out) pred_out[(row * C + ref_idx) * 2 * N + i] = v;
                if (tgt_out) tgt_out[(row * C + ref_idx) * 2 * N + i] = v;
            }
        }
    }
    __syncthreads();
    if (!live || !p2cp_mm) return;
    if (!valid) {
        if (lane == 0) p2cp_mm[tile] = 0.f;
        return;
    }
    float su = 0.f, sv = 0.f;
    for (int i = lane; i < N; i += 64) su += sqrtf(as_p2cp_scan(px[i], py[i], tx, ty, N4));   // prediction -> closest target point
    for (int j = lane; j < N; j += 64) sv += sqrtf(as_p2cp_scan(tx[j], ty[j], px, py, N4));   // target -> closest prediction point
    su = as_wave_sum(su);
    sv = as_wave_sum(sv);
    if (lane == 0) p2cp_mm[tile] = ((su / N + sv / N) * 0.5f) * to_mm;
}

// st [5][A]: count | mean | M2 | min | max.  Lane l takes the rows l, l + 64, ...; the butterfly adds the 64 partials in one order.
__global__ __launch_bounds__(256) void pc_eval_errors_kernel(const float* __restrict__ e, int A, int64_t rows,
                                                             const int32_t* __restrict__ lengths, int T, double* __restrict__ st) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + wave;
    if (a >= A) return;
    double s = 0.0, m = 0.0;
    for (int64_t r = lane; r < rows; r += 64)
        if (pce_valid(lengths, T, r)) { s += (double)e[r * A + a]; m += 1.0; }
    s = as_wave_sum_d(s);
    m = as_wave_sum_d(m);
    if (m == 0.0) return;
    const double bmean = s / m;
    double q = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t r = lane; r < rows; r += 64)
        if (pce_valid(lengths, T, r)) {
            const double x = (double)e[r * A + a], d = x - bmean;
            q = fma(d, d, q);
            mn = fmin(mn, x);
            mx = fmax(mx, x);
        }
    q = as_wave_sum_d(q);
    mn = as_wave_min_d(mn);
    mx = as_wave_max_d(mx);
    if (lane != 0) return;
    const double n = st[a], nn = n + m, delta = bmean - st[A + a];
    st[2 * A + a] = st[2 * A + a] + q + delta * delta * (n * m / nn);
    st[A + a] = st[A + a] + delta * (m / nn);
    st[3 * A + a] = n == 0.0 ? mn : fmin(st[3 * A + a], mn);
    st[4 * A + a] = n == 0.0 ? mx : fmax(st[4 * A + a], mx);
    st[a] = nn;
}

// st = count | mean [L] | M2 [L][L].  One workgroup of 256: column sums over 4 row partitions (row r belongs to partition r % 4),
// then every thread owns up to PCE_PAIRS entries of the matrix and adds the rows' centred products in row order.
__global__ __launch_bounds__(256) void pc_eval_latents_kernel(const float* __restrict__ x, int L, int64_t rows,
                                                              const int32_t* __restrict__ lengths, int T, double* __restrict__ st) {
    __shared__ double s_d[PCE_CHUNK][PCE_MAX_L];
    __shared__ double s_part[4][PCE_MAX_L], s_bmean[PCE_MAX_L], s_delta[PCE_MAX_L], s_cnt[4];
    const int tid = threadIdx.x, j = tid & 63, part = tid >> 6, LL = L * L;
    double s = 0.0, c = 0.0;
    for (int64_t r = part; r < rows; r += 4)
        if (pce_valid(lengths, T, r)) {
            if (j < L) s += (double)x[r * L + j];
            c += 1.0;
        }
    s_part[part][j] = s;
    if (j == 0) s_cnt[part] = c;
    __syncthreads();
    const double m = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    if (m == 0.0) return;
    if (tid < L) s_bmean[tid] = ((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) / m;
    __syncthreads();

    double acc[PCE_PAIRS];
#pragma unroll
    for (int k = 0; k < PCE_PAIRS; ++k) acc[k] = 0.0;
    for (int64_t r0 = 0; r0 < rows; r0 += PCE_CHUNK) {
        for (int e = tid; e < PCE_CHUNK * L; e += 256) {
            const int rr = e / L, jj = e % L;
            const int64_t r = r0 + rr;
            s_d[rr][jj] = (r < rows && pce_valid(lengths, T, r)) ? (double)x[r * L + jj] - s_bmean[jj] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PCE_PAIRS; ++k) {
            const int e = tid + k * 256;
            if (e < LL) {
                const int p = e / L, q = e % L;
                double v = acc[k];
                for (int rr = 0; rr < PCE_CHUNK; ++rr) v = fma(s_d[rr][p], s_d[rr][q], v);
                acc[k] = v;
            }
        }
        __syncthreads();
    }

    const double n = st[0], nn = n + m, w = n * m / nn;
    double* mean = st + 1;
    double* M2 = st + 1 + L;
    if (tid < L) s_delta[tid] = s_bmean[tid] - mean[tid];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PCE_PAIRS; ++k) {
        const int e = tid + k * 256;
        if (e < LL) M2[e] = M2[e] + acc[k] + s_delta[e / L] * s_delta[e % L] * w;
    }
    if (tid < L) mean[tid] = mean[tid] + s_delta[tid] * (m / nn);
    if (tid == 0) st[0] = nn;
}

int pce_check_rows(const char* who, int64_t rows, const int32_t* lengths, int32_t T) {
    AS_REQUIRE(rows > 0, AS_ERR_BAD_ARG, "%s: rows must be positive", who);
    AS_REQUIRE(!lengths || (T > 0 && rows % T == 0), AS_ERR_BAD_ARG, "%s: with lengths, rows (%lld) must be a multiple of T (%d)", who,
               (long long)rows, T);
    return 0;
}

}  // namespace

extern "C" int as_pc_shapes_eval(const float* shapes, const float* targets, const float* mean, const float* std,
                                 const int32_t* lengths, int32_t T, const float* reference, int32_t ref_idx, int64_t rows, int32_t A,
                                 int32_t N, float to_mm, float* pred_out, float* tgt_out, float* p2cp_mm, void* stream) {
    AS_REQUIRE(shapes && targets && mean && std && A >= 1 && N >= 1, AS_ERR_BAD_ARG, "as_pc_shapes_eval: bad argument");
    AS_TRY(pce_check_rows("as_pc_shapes_eval", rows, lengths, T));
    AS_REQUIRE(ref_idx >= -1 && ref_idx <= A && (ref_idx < 0 || reference), AS_ERR_BAD_ARG,
               "as_pc_shapes_eval: ref_idx %d must be -1 or in [0, %d] with a reference array", ref_idx, A);
    AS_REQUIRE(N <= PCE_MAX_N, AS_ERR_UNSUPPORTED, "as_pc_shapes_eval: %d points per contour, at most %d", N, PCE_MAX_N);
    const int64_t tiles = rows * A;
    AS_REQUIRE(tiles / 4 < 0x7fffffffLL, AS_ERR_UNSUPPORTED, "as_pc_shapes_eval: %lld tiles exceed one grid", (long long)tiles);
    if (!pred_out && !tgt_out && !p2cp_mm) return 0;
    hipLaunchKernelGGL(pc_shapes_eval_kernel, dim3(as_cdiv(tiles, 4)), dim3(256), 0, (hipStream_t)stream, shapes, targets, mean, std,
                       lengths, T, reference, ref_idx, tiles, A, N, to_mm, pred_out, tgt_out, p2cp_mm);
    AS_LAUNCH_CHECK("as_pc_shapes_eval");
    return 0;
}

extern "C" int as_pc_eval_accumulate(const float* p2cp_mm, int32_t A, double* err_state, const float* latents, int32_t L,
                                     double* lat_state, int64_t rows, const int32_t* lengths, int32_t T, void* stream) {
    AS_TRY(pce_check_rows("as_pc_eval_accumulate", rows, lengths, T));
    AS_REQUIRE(!p2cp_mm || (err_state && A >= 1), AS_ERR_BAD_ARG, "as_pc_eval_accumulate: errors need a state and A >= 1");
    AS_REQUIRE(!latents || (lat_state && L >= 1), AS_ERR_BAD_ARG, "as_pc_eval_accumulate: latents need a state and L >= 1");
    AS_REQUIRE(!latents || L <= PCE_MAX_L, AS_ERR_UNSUPPORTED, "as_pc_eval_accumulate: latent size %d, at most %d", L, PCE_MAX_L);
    if (p2cp_mm) {
        hipLaunchKernelGGL(pc_eval_errors_kernel, dim3(as_cdiv(A, 4)), dim3(256), 0, (hipStream_t)stream, p2cp_mm, A, rows, lengths,
                           T, err_state);
        AS_LAUNCH_CHECK("as_pc_eval_accumulate (errors)");
    }
    if (latents) {
        hipLaunchKernelGGL(pc_eval_latents_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, latents, L, rows, lengths, T,
                           lat_state);
        AS_LAUNCH_CHECK("as_pc_eval_accumulate (latents)");
    }
    return 0;
}
