// Exact t-SNE on the device (reference phoneme_recognition/__init__.py:355-356: sklearn.manifold.TSNE(n_components=2)
// .fit_transform on the recogniser's last hidden features).  Four stages, every one of them free of float atomics and with every
// cross-workgroup sum taken from a workspace in a fixed order, so that equal inputs give equal bits:
//
//   as_tsne_sqdist    ts_sqdist_kernel: a 64 x 64 tile of the (N, N) squared distances per workgroup of 256 threads, 4 x 4 outputs
//                     per thread, X staged through LDS 32 columns at a time.  dist[i][j] = sum_k (x_ik - x_jk)^2 by direct
//                     differences in ONE float32 chain over k: (a - b)^2 == (b - a)^2 bit for bit and both sides add in the same
//                     order, so the matrix is exactly symmetric, and x_i - x_i = 0 leaves an exactly zero diagonal.
//   as_tsne_joint_p   ts_bisect_kernel: one wave per row, scikit-learn's _binary_search_perplexity in float64 (start at beta = 1, at
//                     most 100 steps, |H - log perplexity| <= 1e-5, its interval-doubling rule); the row of distances is read
//                     from L2 on every step.  ts_total_kernel adds the rows' sums of conditional probabilities in row order;
//                     ts_symmetrize_kernel rebuilds the two conditional probabilities of a pair from (beta, sum) of its two rows --
//                     always the lower row first, so that P[i][j] and P[j][i] are the same expression -- and stores
//                     max((c_ij + c_ji) / max(total, eps), eps) as float32 with a zero diagonal.
//   as_tsne_iterate   per iteration ts_pair_kernel + ts_update_kernel, enqueued back to back with no host synchronisation.
//                     The pair pass reads P through its symmetry: a thread owns point i and walks the rows j of its slab, so the
//                     64 lanes of a wave read 64 consecutive floats of row j (P[j][i] == P[i][j]), y_j is one LDS broadcast, and
//                     the five sums of point i stay in the thread's registers (float64): no cross-lane reduction in the loop.
//                     The grid is (tiles of 256 points) x (slabs of rows); a workgroup writes its points' attractive and repulsive
//                     partial sums per (slab, point) and ONE partial of Z = sum num.  The update kernel adds the workgroups' Z in
//                     workgroup order (every workgroup does, to the same bits), the slabs of its points in slab order, forms
//                     4 (e attr - rep / Z) and applies scikit-learn's _gradient_descent step; the workgroups' squared gradient
//                     norms are added in workgroup order by whichever workgroup draws the last integer ticket (frame_ce.hip's
//                     hand-over: nobody waits on it).
//   (KL)              where asked: the update kernel keeps the Y it started from and Z, ts_kl_kernel walks the pairs once more in
//                     float64 and ts_kl_finish_kernel adds the workgroups' partial sums in workgroup order.
#include <math.h>

#include "as_common.h"
#include "as_device.h"
#include "as_launch.h"

namespace {

constexpr int TS_MAX_N = 16384;        // points: the (N, N) float32 matrices reach 1 GiB each
constexpr int TS_TILE = 256;           // points of one pair-pass workgroup, one per thread
constexpr int TS_MIN_SLAB_ROWS = 16;   // rows of a slab: no fewer (a slab is one pass over its Y in LDS)
constexpr int TS_MAX_SLAB_ROWS = 2048; // and no more: 16 KiB of LDS
constexpr int TS_MAX_SLABS = 64;
constexpr int TS_TARGET_WGS = 768;     // three pair-pass workgroups per CU
constexpr int TS_DT = 64, TS_DK = 32;  // distance tile and its k-chunk
constexpr double TS_EPS = 2.220446049250313e-16;   // np.finfo(np.double).eps: scikit-learn's MACHINE_EPSILON

struct TsPlan { int tiles, rows, slabs; };

// The pair pass of N points: tiles of 256 points times slabs of `rows` rows.  The slab count aims at TS_TARGET_WGS workgroups
// and depends on N alone, so the order of every sum does too.
TsPlan ts_plan(int N) {
    TsPlan p;
    p.tiles = as_cdiv(N, TS_TILE);
    int target = as_cdiv(TS_TARGET_WGS, p.tiles);
    target = target < 1 ? 1 : (target > TS_MAX_SLABS ? TS_MAX_SLABS : target);
    p.rows = as_cdiv(N, target);
    if (p.rows < TS_MIN_SLAB_ROWS) p.rows = TS_MIN_SLAB_ROWS;
    p.slabs = as_cdiv(N, p.rows);
    return p;
}

// workspace carve (bytes from its start; every region 16-byte aligned)
struct TsWs { int64_t head, zwg, klwg, gn, part, yold, rsum, rtot, end; };
TsWs ts_carve(int N) {
    const TsPlan p = ts_plan(N);
    const int64_t wgs = (int64_t)p.tiles * p.slabs;
    TsWs w;
    w.head = 0;                                          // [0] ticket (uint64), [1] Z, [2] total of the conditional P (doubles)
    w.zwg = 64;                                          // Z partial per pair-pass workgroup
    w.klwg = w.zwg + as_round_up(8 * wgs, 16);           // KL partial per workgroup
    w.gn = w.klwg + as_round_up(8 * wgs, 16);            // (|grad|^2, |gains grad|^2) per update workgroup
    w.part = w.gn + 16 * (int64_t)p.tiles;               // float [slab][4][N]
    w.yold = w.part + as_round_up(16LL * p.slabs * N, 16);   // float [N][2]
    w.rsum = w.yold + as_round_up(8LL * N, 16);          // joint_p: double [N] sum_j exp(-d beta) of a row
    w.rtot = w.rsum + as_round_up(8LL * N, 16);          // joint_p: double [N] the row's conditional probabilities added up
    w.end = w.rtot + as_round_up(8LL * N, 16);
    return w;
}

// ---- (a) squared distances
__global__ __launch_bounds__(256) void ts_sqdist_kernel(const float* __restrict__ x, long ldx, int N, int D, float* __restrict__ dist) {
    __shared__ float sa[TS_DT][TS_DK + 1], sb[TS_DT][TS_DK + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * TS_DT, j0 = blockIdx.x * TS_DT;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < D; k0 += TS_DK) {
        const int c = tid & 31, k = k0 + c;
#pragma unroll
        for (int r = tid >> 5; r < TS_DT; r += 8) {   // 32 consecutive floats of a row per 32 lanes; zero past N and D
            const int i = i0 + r, j = j0 + r;
            sa[r][c] = (i < N && k < D) ? x[i * ldx + k] : 0.f;
            sb[r][c] = (j < N && k < D) ? x[j * ldx + k] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < TS_DK; ++kk) {   // a padded column adds (0 - 0)^2: the chain's value is unchanged
            float a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = sa[ty + 16 * u][kk];
                b[u] = sb[tx + 16 * u][kk];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float d = a[u] - b[v];
                    acc[u][v] = fmaf(d, d, acc[u][v]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
            if (i < N && j < N) dist[(long)i * N + j] = i == j ? 0.f : acc[u][v];
        }
}

// ---- (b) joint probabilities
// One wave per row.  beta, H and sum are those of the LAST evaluation (scikit-learn's row of conditional probabilities is the
// one of that evaluation too: after its 100th step it moves beta once more and never uses it).
__global__ __launch_bounds__(256) void ts_bisect_kernel(const float* __restrict__ dist, int N, double log_perp, double* __restrict__ beta_out,
                                                        double* __restrict__ h_out, int* __restrict__ steps_out,
                                                        double* __restrict__ rsum, double* __restrict__ rtot) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;   // wave-uniform; the kernel has no barrier
    const float* __restrict__ d = dist + (long)row * N;
    double beta = 1.0, bmin = -INFINITY, bmax = INFINITY, h = 0.0, s = 0.0;
    int step = 1;
    for (;; ++step) {
        double sp = 0.0, sd = 0.0;
        for (int j = lane; j < N; j += 64) {
            if (j == row) continue;
            const double dj = (double)d[j], e = exp(-dj * beta);
            sp += e;
            sd += dj * e;
        }
        sp = as_wave_sum_d(sp);
        sd = as_wave_sum_d(sd);
        if (sp == 0.0) sp = 1e-8;   // EPSILON_DBL of _binary_search_perplexity
        s = sp;
        h = log(sp) + beta * (sd / sp);
        const double diff = h - log_perp;
        if (fabs(diff) <= 1e-5 || step == 100) break;
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == INFINITY ? beta * 2.0 : (beta + bmax) / 2.0;
        } else {
            bmax = beta;
            beta = bmin == -INFINITY ? beta / 2.0 : (beta + bmin) / 2.0;
        }
    }
    double t = 0.0;
    for (int j = lane; j < N; j += 64)
        if (j != row) t += exp(-(double)d[j] * beta) / s;
    t = as_wave_sum_d(t);
    if (lane == 0) {
        beta_out[row] = beta;
        h_out[row] = h;
        steps_out[row] = step;
        rsum[row] = s;
        rtot[row] = t;
    }
}

// sum over a workgroup of 256 threads, the same value in every thread: the lanes of a wave by butterfly, the four waves in order
__device__ __forceinline__ double ts_block_sum(double v, double* sh4) {
    v = as_wave_sum_d(v);
    __syncthreads();   // sh4 may still be read from a previous sum
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// head[2] = max(sum(C + C'), eps) = max(2 sum_i rtot[i], eps): one workgroup, thread t adds rows t, t + 256, ... in order
__global__ __launch_bounds__(256) void ts_total_kernel(const double* __restrict__ rtot, int N, double* __restrict__ head) {
    __shared__ double sh4[4];
    double t = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) t += rtot[i];
    t = 2.0 * ts_block_sum(t, sh4);
    if (threadIdx.x == 0) head[2] = fmax(t, TS_EPS);
}

__global__ __launch_bounds__(256) void ts_symmetrize_kernel(const float* __restrict__ dist, int N, const double* __restrict__ beta,
                                                            const double* __restrict__ rsum, const double* __restrict__ head,
                                                            float* __restrict__ P) {
    const int i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    float p = 0.f;
    if (i != j) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;   // one expression for (i, j) and (j, i)
        const double d = (double)dist[(long)i * N + j];
        const double c_lo = exp(-d * beta[lo]) / rsum[lo], c_hi = exp(-d * beta[hi]) / rsum[hi];
        p = (float)fmax((c_lo + c_hi) / head[2], TS_EPS);
    }
    P[(long)i * N + j] = p;
}

// ---- (c) pair pass
__global__ __launch_bounds__(TS_TILE) void ts_pair_kernel(const float* __restrict__ P, const float2* __restrict__ Y, int N, int rows,
                                                          float* __restrict__ part, double* __restrict__ zwg) {
    __shared__ float2 sh_y[TS_MAX_SLAB_ROWS];
    __shared__ double sh4[4];
    const int i = blockIdx.x * TS_TILE + threadIdx.x, slab = blockIdx.y;
    const int j0 = slab * rows, nj = min(N - j0, rows);
    for (int k = threadIdx.x; k < nj; k += TS_TILE) sh_y[k] = Y[j0 + k];
    __syncthreads();
    double z = 0.0, ax = 0.0, ay = 0.0, rx = 0.0, ry = 0.0;
    if (i < N) {
        const float2 yi = Y[i];
        const float* __restrict__ p = P + (long)j0 * N + i;   // P[j][i] == P[i][j]: consecutive lanes, consecutive floats
#pragma unroll 8
        for (int k = 0; k < nj; ++k) {
            const float pij = p[(long)k * N];
            const float2 yj = sh_y[k];
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            float num = 1.0f / (1.0f + (dx * dx + dy * dy));   // an IEEE division
            if (j0 + k == i) num = 0.f;
            const float pn = pij * num, n2 = num * num;
            z += (double)num;
            ax += (double)(pn * dx);
            ay += (double)(pn * dy);
            rx += (double)(n2 * dx);
            ry += (double)(n2 * dy);
        }
        float* __restrict__ o = part + (long)slab * 4 * N + i;
        o[0] = (float)ax;
        o[N] = (float)ay;
        o[2L * N] = (float)rx;
        o[3L * N] = (float)ry;
    }
    z = ts_block_sum(z, sh4);
    if (threadIdx.x == 0) zwg[blockIdx.y * gridDim.x + blockIdx.x] = z;
}

// ---- (d) update
// log_row: (|grad|, |gains grad|, KL): the first two from here, the third NaN unless the KL pass of this iteration follows
// (keep != 0: Y as it was and Z are kept for it).
__global__ __launch_bounds__(TS_TILE) void ts_update_kernel(const float* __restrict__ part, const double* __restrict__ zwg, int wgs, int N,
                                                            int slabs, float2* __restrict__ Y, float2* __restrict__ upd,
                                                            float2* __restrict__ gains, float exaggeration, float momentum, float lr,
                                                            float min_gain, float2* __restrict__ grad_out, int keep,
                                                            float2* __restrict__ yold, double* head, unsigned long long* gn,
                                                            double* __restrict__ log_row) {
    __shared__ double sh4[4];
    double zt = 0.0;
    for (int w = threadIdx.x; w < wgs; w += TS_TILE) zt += zwg[w];
    const double Z = ts_block_sum(zt, sh4);   // the same bits in every workgroup
    const int i = blockIdx.x * TS_TILE + threadIdx.x;
    double g2 = 0.0, gg2 = 0.0;
    if (i < N) {
        double ax = 0.0, ay = 0.0, rx = 0.0, ry = 0.0;
        for (int s = 0; s < slabs; ++s) {
            const float* __restrict__ o = part + (long)s * 4 * N + i;
            ax += (double)o[0];
            ay += (double)o[N];
            rx += (double)o[2L * N];
            ry += (double)o[3L * N];
        }
        const float gx = (float)(4.0 * ((double)exaggeration * ax - rx / Z)), gy = (float)(4.0 * ((double)exaggeration * ay - ry / Z));
        float2 y = Y[i], u = upd[i], g = gains[i];
        if (keep) yold[i] = y;
        if (grad_out) grad_out[i] = make_float2(gx, gy);
        g.x = fmaxf(u.x * gx < 0.f ? g.x + 0.2f : g.x * 0.8f, min_gain);
        g.y = fmaxf(u.y * gy < 0.f ? g.y + 0.2f : g.y * 0.8f, min_gain);
        const float ggx = g.x * gx, ggy = g.y * gy;
        u.x = momentum * u.x - lr * ggx;
        u.y = momentum * u.y - lr * ggy;
        y.x += u.x;
        y.y += u.y;
        gains[i] = g;
        upd[i] = u;
        Y[i] = y;
        g2 = (double)gx * gx + (double)gy * gy;
        gg2 = (double)ggx * ggx + (double)ggy * ggy;
    }
    g2 = ts_block_sum(g2, sh4);
    gg2 = ts_block_sum(gg2, sh4);
    if (threadIdx.x != 0) return;
    if (keep && blockIdx.x == 0) head[1] = Z;
    unsigned long long* ticket = reinterpret_cast<unsigned long long*>(head);
    __hip_atomic_store(gn + 2 * blockIdx.x, (unsigned long long)__double_as_longlong(g2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(gn + 2 * blockIdx.x + 1, (unsigned long long)__double_as_longlong(gg2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // this thread alone stored the pair (write-through agent-scope stores): drained before the ticket says so
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t = __hip_atomic_fetch_add(ticket, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t != gridDim.x - 1) return;
    __threadfence();   // the last workgroup: every pair is read by an agent-scope load, added in workgroup order
    g2 = gg2 = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) {
        g2 += __longlong_as_double((long long)__hip_atomic_load(gn + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        gg2 += __longlong_as_double((long long)__hip_atomic_load(gn + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    log_row[0] = sqrt(g2);
    log_row[1] = sqrt(gg2);
    if (!keep) log_row[2] = NAN;
    __hip_atomic_store(ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch finds the ticket at zero
}

// ---- (e) KL divergence of the kept Y: sum over the ordered pairs i != j = 2 sum_{i<j}, in float64
__global__ __launch_bounds__(TS_TILE) void ts_kl_kernel(const float* __restrict__ P, const float2* __restrict__ Y, const double* __restrict__ head,
                                                        int N, int rows, double* __restrict__ klwg) {
    __shared__ float2 sh_y[TS_MAX_SLAB_ROWS];
    __shared__ double sh4[4];
    const int i = blockIdx.x * TS_TILE + threadIdx.x, slab = blockIdx.y;
    const int j0 = slab * rows, nj = min(N - j0, rows);
    for (int k = threadIdx.x; k < nj; k += TS_TILE) sh_y[k] = Y[j0 + k];
    __syncthreads();
    const double Z = head[1];
    double kl = 0.0;
    if (i < N) {
        const float2 yi = Y[i];
        const float* __restrict__ p = P + (long)j0 * N + i;
        for (int k = 0; k < nj; ++k) {
            if (j0 + k == i) continue;
            const double pij = (double)p[(long)k * N];
            const float2 yj = sh_y[k];
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            const double q = fmax((double)(1.0f / (1.0f + (dx * dx + dy * dy))) / Z, TS_EPS);
            kl += pij * log(fmax(pij, TS_EPS) / q);
        }
    }
    kl = ts_block_sum(kl, sh4);
    if (threadIdx.x == 0) klwg[blockIdx.y * gridDim.x + blockIdx.x] = kl;
}

__global__ __launch_bounds__(256) void ts_kl_finish_kernel(const double* __restrict__ klwg, int wgs, double* __restrict__ log_row) {
    __shared__ double sh4[4];
    double t = 0.0;
    for (int w = threadIdx.x; w < wgs; w += 256) t += klwg[w];
    t = ts_block_sum(t, sh4);
    if (threadIdx.x == 0) log_row[2] = t;
}

int ts_check_n(const char* who, int32_t N) {
    AS_REQUIRE(N >= 2, AS_ERR_BAD_ARG, "%s: N = %d, at least 2 points are needed", who, N);
    AS_REQUIRE(N <= TS_MAX_N, AS_ERR_BAD_ARG, "%s: N = %d, at most %d points are supported", who, N, TS_MAX_N);
    return 0;
}

int ts_check_ws(const char* who, int32_t N, const void* ws, int64_t ws_bytes) {
    const int64_t need = as_tsne_workspace_bytes(N);
    AS_REQUIRE(ws && ws_bytes >= need && as_aligned16(ws), AS_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed (16-byte aligned)",
               who, (long long)(ws ? ws_bytes : 0), (long long)need);
    return 0;
}

}  // namespace

extern "C" int64_t as_tsne_workspace_bytes(int32_t N) {
    if (N < 2 || N > TS_MAX_N) return 0;
    return ts_carve(N).end;
}

extern "C" int as_tsne_sqdist(const float* x, int64_t ldx, int32_t N, int32_t D, float* dist, void* stream) {
    AS_REQUIRE(x && dist, AS_ERR_BAD_ARG, "as_tsne_sqdist: bad argument (null pointer)");
    AS_TRY(ts_check_n("as_tsne_sqdist", N));
    AS_REQUIRE(D >= 1 && ldx >= D, AS_ERR_BAD_ARG, "as_tsne_sqdist: bad argument (D = %d, row stride %lld)", D, (long long)ldx);
    const int t = as_cdiv(N, TS_DT);
    hipLaunchKernelGGL(ts_sqdist_kernel, dim3(t, t), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, N, D, dist);
    AS_LAUNCH_CHECK("as_tsne_sqdist");
    return 0;
}

extern "C" int as_tsne_joint_p(const float* dist, int32_t N, double perplexity, float* P, double* beta, double* entropy, int32_t* steps,
                               void* ws, int64_t ws_bytes, void* stream) {
    AS_REQUIRE(dist && P && beta && entropy && steps, AS_ERR_BAD_ARG, "as_tsne_joint_p: bad argument (null pointer)");
    AS_TRY(ts_check_n("as_tsne_joint_p", N));
    AS_REQUIRE(perplexity > 0.0 && perplexity < (double)N, AS_ERR_BAD_ARG, "as_tsne_joint_p: perplexity %g outside (0, N = %d)", perplexity,
               N);
    AS_TRY(ts_check_ws("as_tsne_joint_p", N, ws, ws_bytes));
    const TsWs w = ts_carve(N);
    char* base = static_cast<char*>(ws);
    double* head = reinterpret_cast<double*>(base + w.head);
    double* rsum = reinterpret_cast<double*>(base + w.rsum);
    double* rtot = reinterpret_cast<double*>(base + w.rtot);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ts_bisect_kernel, dim3(as_cdiv(N, 4)), dim3(256), 0, st, dist, N, log(perplexity), beta, entropy, steps, rsum, rtot);
    AS_LAUNCH_CHECK("as_tsne_joint_p");
    hipLaunchKernelGGL(ts_total_kernel, dim3(1), dim3(256), 0, st, rtot, N, head);
    AS_LAUNCH_CHECK("as_tsne_joint_p");
    hipLaunchKernelGGL(ts_symmetrize_kernel, dim3(as_cdiv(N, 256), N), dim3(256), 0, st, dist, N, beta, rsum, head, P);
    AS_LAUNCH_CHECK("as_tsne_joint_p");
    return 0;
}

extern "C" int as_tsne_iterate(const float* P, float* Y, float* update, float* gains, int32_t N, int32_t n_iters, int32_t it0,
                               int32_t kl_every, int32_t kl_last, float exaggeration, float momentum, float learning_rate, float min_gain,
                               float* grad, double* log, void* ws, int64_t ws_bytes, void* stream) {
    AS_REQUIRE(P && Y && update && gains && log, AS_ERR_BAD_ARG, "as_tsne_iterate: bad argument (null pointer)");
    AS_REQUIRE(((uintptr_t)Y | (uintptr_t)update | (uintptr_t)gains | (uintptr_t)grad | (uintptr_t)log) % 8 == 0, AS_ERR_BAD_ARG,
               "as_tsne_iterate: bad argument (Y, update, gains, grad and log must be 8-byte aligned)");
    AS_TRY(ts_check_n("as_tsne_iterate", N));
    AS_REQUIRE(n_iters >= 1 && it0 >= 0 && kl_every >= 0, AS_ERR_BAD_ARG, "as_tsne_iterate: bad argument (n_iters = %d, it0 = %d, kl_every = %d)",
               n_iters, it0, kl_every);
    AS_TRY(ts_check_ws("as_tsne_iterate", N, ws, ws_bytes));
    const TsPlan p = ts_plan(N);
    AS_REQUIRE(p.rows <= TS_MAX_SLAB_ROWS, AS_ERR_BAD_ARG, "as_tsne_iterate: N = %d needs slabs of %d rows (at most %d)", N, p.rows,
               TS_MAX_SLAB_ROWS);
    const TsWs w = ts_carve(N);
    char* base = static_cast<char*>(ws);
    double* head = reinterpret_cast<double*>(base + w.head);
    double* zwg = reinterpret_cast<double*>(base + w.zwg);
    double* klwg = reinterpret_cast<double*>(base + w.klwg);
    unsigned long long* gn = reinterpret_cast<unsigned long long*>(base + w.gn);
    float* part = reinterpret_cast<float*>(base + w.part);
    float2* yold = reinterpret_cast<float2*>(base + w.yold);
    hipStream_t st = (hipStream_t)stream;
    const int wgs = p.tiles * p.slabs;
    const hipError_t e = hipMemsetAsync(head, 0, 8, st);   // the ticket starts every call at zero, whatever the workspace held
    AS_REQUIRE(e == hipSuccess, (int)e, "as_tsne_iterate: clearing the ticket failed: %s", hipGetErrorString(e));
    for (int k = 0; k < n_iters; ++k) {
        const int keep = (kl_every > 0 && (it0 + k + 1) % kl_every == 0) || (kl_last && k == n_iters - 1);
        double* log_row = log + 3L * k;
        hipLaunchKernelGGL(ts_pair_kernel, dim3(p.tiles, p.slabs), dim3(TS_TILE), 0, st, P, reinterpret_cast<const float2*>(Y), N, p.rows,
                           part, zwg);
        AS_LAUNCH_CHECK("as_tsne_iterate");
        hipLaunchKernelGGL(ts_update_kernel, dim3(p.tiles), dim3(TS_TILE), 0, st, part, zwg, wgs, N, p.slabs, reinterpret_cast<float2*>(Y),
                           reinterpret_cast<float2*>(update), reinterpret_cast<float2*>(gains), exaggeration, momentum, learning_rate,
                           min_gain, reinterpret_cast<float2*>(grad), keep, yold, head, gn, log_row);
        AS_LAUNCH_CHECK("as_tsne_iterate");
        if (keep) {
            hipLaunchKernelGGL(ts_kl_kernel, dim3(p.tiles, p.slabs), dim3(TS_TILE), 0, st, P, yold, head, N, p.rows, klwg);
            AS_LAUNCH_CHECK("as_tsne_iterate");
            hipLaunchKernelGGL(ts_kl_finish_kernel, dim3(1), dim3(256), 0, st, klwg, wgs, log_row);
            AS_LAUNCH_CHECK("as_tsne_iterate");
        }
    }
    return 0;
}
