// MeanP2CPDistance as a loss (reference phoneme_to_articulation/metrics.py:27-46, differentiated there through torch.cdist and
// min): the gradient of metrics.hip's p2cp_kernel, and the length-masked mean of the criterion with its gradient in one pass
// (the twin of euclid_masked_kernel; train_phoneme_to_articulation.py:86-90).
//
// One wave per (u, v) tile, four tiles per workgroup, as the forward has.  Both point sets are staged in LDS once; lane i finds
// the closest v point of u_i, lane j the closest u point of v_j -- as_p2cp_scan_argmin, the forward's squared distances from
// the forward's expression, lowest index among equals -- and the two index arrays go to LDS next to the points.  Then the lane
// that owns point i gathers its terms: its own closest point, plus every point of the other set that chose i, in ascending
// index order.  A gather, not a scatter: no atomics, no state kept from the forward, and a run repeats bit for bit.
//   d |a - b| / d a = e(a, b) = (a - b) / |a - b|, and 0 where the two coincide (cdist's backward), so
//   du_i = dout * ( e(u_i, v_j*(i)) / (2 n_u) + sum_{j : i*(j) = i} e(u_i, v_j) / (2 n_v) ), dv_j the mirror image.
// Built with -ffp-contract=off like metrics.hip: the closest points are those of the un-contracted forward.
#include "as_device.h"
#include "gemm_internal.h"

namespace {

constexpr int P2CP_MAXPTS = 256;         // points per side, as as_p2cp_fwd
constexpr int P2CP_LOSS_BLOCKS = 2048;   // workgroup partials of the masked criterion (8 workgroups per compute unit)

struct P2cpTile {
    float *ux, *uy, *vx, *vy;   // the points, padded to a multiple of 4 with +inf: a padding point is never a minimum
    int *ri, *ci;               // ri[i] = j*(i), ci[j] = i*(j); padded with -1: a padding entry chooses nobody
};

__device__ __forceinline__ P2cpTile p2cp_tile_lds(float* smem, int wave, int nu4, int nv4) {
    P2cpTile t;
    t.ux = smem + (long)wave * 3 * (nu4 + nv4);
    t.uy = t.ux + nu4;
    t.vx = t.uy + nu4;
    t.vy = t.vx + nv4;
    t.ri = reinterpret_cast<int*>(t.vy + nv4);
    t.ci = t.ri + nu4;
    return t;
}

__device__ __forceinline__ void p2cp_stage(const P2cpTile& t, int lane, const float* __restrict__ up, long u_pt, long u_xy, int nu,
                                           int nu4, const float* __restrict__ vp, long v_pt, long v_xy, int nv, int nv4) {
    for (int i = lane; i < nu4; i += 64) {
        t.ux[i] = i < nu ? up[i * u_pt] : INFINITY;
        t.uy[i] = i < nu ? up[i * u_pt + u_xy] : INFINITY;
        t.ri[i] = -1;
    }
    for (int i = lane; i < nv4; i += 64) {
        t.vx[i] = i < nv ? vp[i * v_pt] : INFINITY;
        t.vy[i] = i < nv ? vp[i * v_pt + v_xy] : INFINITY;
        t.ci[i] = -1;
    }
}

// both closest-point index arrays; returns the tile's P2CP (p2cp_kernel's expression and summation order: the same bits)
template <bool VALUE>
__device__ __forceinline__ float p2cp_closest(const P2cpTile& t, int lane, int nu, int nu4, int nv, int nv4) {
    float su = 0.f, sv = 0.f;
    for (int i = lane; i < nu; i += 64) {   // row minima
        float m;
        t.ri[i] = as_p2cp_scan_argmin(t.ux[i], t.uy[i], t.vx, t.vy, nv4, &m);
        if (VALUE) su += sqrtf(m);
    }
    for (int j = lane; j < nv; j += 64) {   // column minima
        float m;
        t.ci[j] = as_p2cp_scan_argmin(t.vx[j], t.vy[j], t.ux, t.uy, nu4, &m);
        if (VALUE) sv += sqrtf(m);
    }
    if (!VALUE) return 0.f;
    su = as_wave_sum(su);
    sv = as_wave_sum(sv);
    return (su / nu + sv / nv) * 0.5f;
}

__device__ __forceinline__ void p2cp_unit(float dx, float dy, float& ex, float& ey) {
    const float d = sqrtf(dx * dx + dy * dy);
    ex = d == 0.f ? 0.f : dx / d;
    ey = d == 0.f ? 0.f : dy / d;
}

// coef * d p2cp / d p for the n_p points p of one side; q is the other side, pi[i] the closest q point of p_i, qi[j] the
// closest p point of q_j (padded to n_q4 with -1).  e(q_j, p_i) = -e(p_i, q_j) exactly, so the same walk serves both sides.
__device__ __forceinline__ void p2cp_side_grad(int lane, const float* px, const float* py, int n_p, const int* pi, const float* qx,
                                               const float* qy, int n_q, int n_q4, const int* qi, float coef, float* __restrict__ g,
                                               long g_pt, long g_xy) {
    const float rp = 0.5f / n_p, rq = 0.5f / n_q;
    for (int i = lane; i < n_p; i += 64) {
        const float x = px[i], y = py[i];
        const int own = pi[i];
        float ex, ey;
        p2cp_unit(x - qx[own], y - qy[own], ex, ey);
        float sx = 0.f, sy = 0.f;
        for (int j = 0; j < n_q4; j += 4) {   // ascending j: the order of the sum is fixed
            const int4 k = *reinterpret_cast<const int4*>(qi + j);
            const int ks[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (ks[c] == i) {
                    float fx, fy;
                    p2cp_unit(x - qx[j + c], y - qy[j + c], fx, fy);
                    sx += fx;
                    sy += fy;
                }
        }
        g[i * g_pt] = coef * (ex * rp + sx * rq);
        g[i * g_pt + g_xy] = coef * (ey * rp + sy * rq);
    }
}

__global__ __launch_bounds__(256) void p2cp_bwd_kernel(const float* __restrict__ u, long u_tile, long u_pt, long u_xy, int nu,
                                                       const float* __restrict__ v, long v_tile, long v_pt, long v_xy, int nv,
                                                       long tiles, const float* __restrict__ dout, float* __restrict__ du,
                                                       long du_tile, long du_pt, long du_xy, float* __restrict__ dv, long dv_tile,
                                                       long dv_pt, long dv_xy) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * 4 + wave;
    const bool live = tile < tiles;
    const int nu4 = (nu + 3) & ~3, nv4 = (nv + 3) & ~3;
    const P2cpTile t = p2cp_tile_lds(smem, wave, nu4, nv4);
    if (live) p2cp_stage(t, lane, u + tile * u_tile, u_pt, u_xy, nu, nu4, v + tile * v_tile, v_pt, v_xy, nv, nv4);
    __syncthreads();
    if (live) p2cp_closest<false>(t, lane, nu, nu4, nv, nv4);
    __syncthreads();
    if (!live) return;
    const float coef = dout[tile];
    if (du) p2cp_side_grad(lane, t.ux, t.uy, nu, t.ri, t.vx, t.vy, nv, nv4, t.ci, coef, du + tile * du_tile, du_pt, du_xy);
    if (dv) p2cp_side_grad(lane, t.vx, t.vy, nv, t.ci, t.ux, t.uy, nu, nu4, t.ri, coef, dv + tile * dv_tile, dv_pt, dv_xy);
}

// tile = (b, t, a): u = out[b][t][a] and v = tgt[b][t][a], both [2][N] (point stride 1, xy stride N).  A workgroup walks
// the tile quads blockIdx.x, blockIdx.x + gridDim.x, ..; each wave keeps the running sum of its tiles, the workgroup writes
// one partial.  A padded frame is never read: its tile adds nothing and its dout is zeroed.
__global__ __launch_bounds__(256) void p2cp_masked_kernel(const float* __restrict__ out, const float* __restrict__ tgt, long tgt_T,
                                                          const int* __restrict__ lengths, int T, int A, int N, long tiles,
                                                          float scale, float* __restrict__ dout, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n4 = (N + 3) & ~3;
    const P2cpTile t = p2cp_tile_lds(smem, wave, n4, n4);
    const long plane = 2L * N;
    float acc = 0.f;
    for (long first = (long)blockIdx.x * 4; first < tiles; first += (long)gridDim.x * 4) {   // the same trip count for all waves
        const long tile = first + wave;
        bool live = false;
        long tgt_at = 0;
        if (tile < tiles) {
            const long frame = tile / A;
            const int a = (int)(tile - frame * A);
            const long b = frame / T;
            const int tt = (int)(frame - b * T);
            live = tt < lengths[b];
            tgt_at = ((b * tgt_T + tt) * A + a) * plane;
        }
        __syncthreads();   // the previous tile's reads are over
        if (live) p2cp_stage(t, lane, out + tile * plane, 1, N, N, n4, tgt + tgt_at, 1, N, N, n4);
        __syncthreads();
        float value = 0.f;
        if (live) value = p2cp_closest<true>(t, lane, N, n4, N, n4);
        __syncthreads();
        acc += value;
        if (dout && tile < tiles) {
            float* g = dout + tile * plane;
            if (live) p2cp_side_grad(lane, t.ux, t.uy, N, t.ri, t.vx, t.vy, N, n4, t.ci, scale, g, 1, N);
            else
                for (int i = lane; i < N; i += 64) g[i] = 0.f, g[N + i] = 0.f;
        }
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

inline size_t p2cp_tile_lds_bytes(int nu, int nv) {
    return (size_t)4 * 3 * (((nu + 3) & ~3) + ((nv + 3) & ~3)) * sizeof(float);
}

}  // namespace

extern "C" int as_p2cp_bwd(const float* u, int64_t u_tile, int64_t u_pt, int64_t u_xy, int32_t n_u, const float* v, int64_t v_tile,
                           int64_t v_pt, int64_t v_xy, int32_t n_v, int64_t tiles, const float* dout, float* du, int64_t du_tile,
                           int64_t du_pt, int64_t du_xy, float* dv, int64_t dv_tile, int64_t dv_pt, int64_t dv_xy, void* stream) {
    AS_REQUIRE(n_u > 0 && n_v > 0 && n_u <= P2CP_MAXPTS && n_v <= P2CP_MAXPTS, AS_ERR_UNSUPPORTED,
               "as_p2cp_bwd: point counts %d, %d must be in [1, %d]", n_u, n_v, P2CP_MAXPTS);
    AS_REQUIRE(u && v && dout && tiles > 0, AS_ERR_BAD_ARG, "as_p2cp_bwd: bad argument");
    if (!du && !dv) return 0;
    hipLaunchKernelGGL(p2cp_bwd_kernel, dim3(as_cdiv(tiles, 4)), dim3(256), p2cp_tile_lds_bytes(n_u, n_v), (hipStream_t)stream, u,
                       (long)u_tile, (long)u_pt, (long)u_xy, n_u, v, (long)v_tile, (long)v_pt, (long)v_xy, n_v, (long)tiles, dout, du,
                       (long)du_tile, (long)du_pt, (long)du_xy, dv, (long)dv_tile, (long)dv_pt, (long)dv_xy);
    AS_LAUNCH_CHECK("as_p2cp_bwd");
    return 0;
}

extern "C" int32_t as_p2cp_masked_partials(void) { return P2CP_LOSS_BLOCKS; }

extern "C" int as_p2cp_masked_fwd_bwd(const float* out, const float* tgt, int64_t tgt_T, const int32_t* lengths, int32_t B, int32_t T,
                                      int32_t A, int32_t N, float scale, float* loss, float* dout, float* partial, void* stream) {
    AS_REQUIRE(out && tgt && lengths && loss && partial, AS_ERR_BAD_ARG, "as_p2cp_masked_fwd_bwd: null pointer");
    AS_REQUIRE(B > 0 && T > 0 && A > 0 && N > 0 && tgt_T >= T, AS_ERR_BAD_ARG, "as_p2cp_masked_fwd_bwd: B=%d T=%d A=%d N=%d tgt_T=%ld", B,
               T, A, N, (long)tgt_T);
    AS_REQUIRE(N <= P2CP_MAXPTS, AS_ERR_UNSUPPORTED, "as_p2cp_masked_fwd_bwd: %d points per contour > %d", N, P2CP_MAXPTS);
    const long tiles = (long)B * T * A;
    long blocks = (tiles + 3) / 4;
    if (blocks > P2CP_LOSS_BLOCKS) blocks = P2CP_LOSS_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(p2cp_masked_kernel, dim3((unsigned)blocks), dim3(256), p2cp_tile_lds_bytes(N, N), st, out, tgt, (long)tgt_T,
                       lengths, T, A, N, tiles, scale, dout, partial);
    AS_LAUNCH_CHECK("as_p2cp_masked_fwd_bwd");
    return as_loss_final(partial, (int)blocks, scale, loss, st);
}
