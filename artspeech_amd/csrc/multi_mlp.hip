// Fused multi-articulator MLPs of the principal-components method (include/artspeech_hip.h: as_multi_mlp_*) and the fused
// masked / weighted MSE of its losses (as_masked_mse_fwd_bwd).
//
// One workgroup per (row tile, articulator) stages that articulator's layers in LDS (W as [out][odd stride], then the bias)
// and runs its whole stack on a tile of MM_RT rows: every hidden activation lives in LDS, nothing but the input rows and the
// output (or the pre-max outputs of the max-scatter mode) touches global memory.  The widths of this method are 2-100, far
// below a matrix-instruction tile, so every dot product is a plain fp32 FMA chain over k in order (exact fp32, no split):
// lane i of the workgroup takes output elements i, i + 256, ... of the tile, n fastest, so the lanes of a wave read distinct
// rows of W (odd stride: distinct banks) and mostly the same activation row (broadcast).
//
// The backward recomputes the hidden activations of its tile from the input (same code, same order: the very values of the
// forward) instead of saving them; one workgroup per (row chunk, articulator) walks the tiles t = chunk, chunk + chunks, ...
// and keeps its weight-gradient partial in a global slot that only its own lanes read and write (fixed order), the chunks
// are summed in chunk order by as_sum_partials.  No float atomics anywhere: two runs are bit-identical.

#include "as_common.h"
#include "as_launch.h"
#include "gemm_internal.h"

namespace {

constexpr int MM_RT = 32;            // rows per tile
constexpr int MM_THREADS = 256;
constexpr int MM_CHUNKS = 32;        // backward workgroups per articulator along the rows (a constant: the dW order depends on R only)
constexpr int MM_MAX_WIDTH = 256;
constexpr int MM_MAX_LDS = 96 * 1024;

__host__ __device__ inline int mm_ld(int w) { return w | 1; }   // odd LDS row stride

struct MMGeo {
    int L, win[3], wout[3];
};

__host__ __device__ inline MMGeo mm_geo(int L, int K, int N, int h1, int h2) {
    MMGeo g;
    g.L = L;
    if (L == 1) {
        g.win[0] = K; g.wout[0] = N;
    } else {
        g.win[0] = K; g.wout[0] = h1;
        g.win[1] = h1; g.wout[1] = h2;
        g.win[2] = h2; g.wout[2] = N;
    }
    return g;
}

// floats of the LDS copy of the layers
__host__ __device__ inline int mm_w_floats(const MMGeo& g) {
    int s = 0;
    for (int l = 0; l < g.L; ++l) s += g.wout[l] * mm_ld(g.win[l]) + g.wout[l];
    return s;
}
__host__ __device__ inline int mm_act_floats(const MMGeo& g) {   // per row: the inputs of every layer
    int s = 0;
    for (int l = 0; l < g.L; ++l) s += mm_ld(g.win[l]);
    return s;
}
__host__ __device__ inline int mm_dz_floats(const MMGeo& g) {    // per row: the output gradients of every layer
    int s = 0;
    for (int l = 0; l < g.L; ++l) s += mm_ld(g.wout[l]);
    return s;
}
// packed gradient slot of one group (geometry of the widest group): W_l [wout][win] then b_l [wout], layer by layer
__host__ __device__ inline int64_t mm_slot_off(const MMGeo& gm, int l) {
    int64_t s = 0;
    for (int i = 0; i < l; ++i) s += (int64_t)gm.wout[i] * gm.win[i] + gm.wout[i];
    return s;
}
inline int64_t mm_lds_bytes(const MMGeo& gm, bool backward) {
    return 4 * ((int64_t)mm_w_floats(gm) + (int64_t)MM_RT * (mm_act_floats(gm) + (backward ? mm_dz_floats(gm) : 0)));
}

struct MMGroup {
    MMGeo geo;
    int K, N;
    float* w[3];     // LDS
    float* b[3];
    float* act[3];   // LDS [MM_RT][mm_ld(win[l])]
};

__device__ inline void mm_group(MMGroup& G, const as_multi_mlp& p, int g, float* lds) {   // G in LDS (thread 0)
    G.K = min(p.dims[2 * g], p.k_max);
    G.N = min(p.dims[2 * g + 1], p.n_max);
    G.geo = mm_geo(p.layers, G.K, G.N, p.h1, p.h2);
    const MMGeo gm = mm_geo(p.layers, p.k_max, p.n_max, p.h1, p.h2);   // LDS offsets from the widest geometry
    float* s = lds;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l < gm.L) {
            G.w[l] = s; s += gm.wout[l] * mm_ld(gm.win[l]);
            G.b[l] = s; s += gm.wout[l];
        }
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (l < gm.L) { G.act[l] = s; s += MM_RT * mm_ld(gm.win[l]); }
    }
}

// the group's W_l [wout][win] (global, contiguous) -> LDS [wout][mm_ld(win)]; a null bias reads as zeros
__device__ inline void mm_stage_weights(const as_multi_mlp& p, int g, const MMGroup& G) {
    for (int l = 0; l < G.geo.L; ++l) {
        const int win = G.geo.win[l], wout = G.geo.wout[l], ld = mm_ld(win);
        const float* W = reinterpret_cast<const float*>(p.params[6 * g + 2 * l]);
        const float* B = reinterpret_cast<const float*>(p.params[6 * g + 2 * l + 1]);
        for (int i = threadIdx.x; i < wout * win; i += MM_THREADS) {
            const int n = i / win, k = i - n * win;
            G.w[l][n * ld + k] = W[i];
        }
        for (int i = threadIdx.x; i < wout; i += MM_THREADS) G.b[l][i] = B ? B[i] : 0.f;
    }
}

// input rows r0 .. r0 + nr of group g -> act[0]
__device__ inline void mm_load_input(const as_multi_mlp& p, int g, const MMGroup& G, int r0, int nr) {
    const int K = G.K, ld = mm_ld(K);
    for (int i = threadIdx.x; i < nr * K; i += MM_THREADS) {
        const int r = i / K, k = i - r * K;
        const int64_t row = (int64_t)(r0 + r) * p.x_r;
        float v;
        if (p.in_mode == 0) {
            v = p.x[row + (int64_t)g * p.x_g + k];
        } else {
            const int j = p.in_idx[g * p.k_max + k];
            v = (unsigned)j < (unsigned)p.latent ? p.in_scale * p.x[row + j] : 0.f;
        }
        G.act[0][r * ld + k] = v;
    }
}

__device__ inline float mm_dot(const float* __restrict__ a, const float* __restrict__ w, int K, float acc) {
    for (int k = 0; k < K; ++k) acc = fmaf(a[k], w[k], acc);
    return acc;
}

// hidden layers: act[l + 1] = ReLU(act[l] W_l^T + b_l), l < L - 1 (ends with a barrier)
__device__ inline void mm_hidden(const MMGroup& G, int nr) {
    for (int l = 0; l + 1 < G.geo.L; ++l) {
        const int win = G.geo.win[l], wout = G.geo.wout[l], ldi = mm_ld(win), ldo = mm_ld(wout);
        for (int i = threadIdx.x; i < nr * wout; i += MM_THREADS) {
            const int r = i / wout, n = i - r * wout;
            G.act[l + 1][r * ldo + n] = as_relu(mm_dot(G.act[l] + r * ldi, G.w[l] + n * ldi, win, 0.f) + G.b[l][n]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(MM_THREADS) void multi_mlp_fwd_kernel(as_multi_mlp p) {
    extern __shared__ float lds[];
    __shared__ MMGroup G;   // in LDS, not registers: the per-layer arrays are indexed by a loop variable
    const int g = blockIdx.y, r0 = blockIdx.x * MM_RT, nr = min(MM_RT, p.rows - r0);
    if (threadIdx.x == 0) mm_group(G, p, g, lds);
    __syncthreads();
    mm_stage_weights(p, g, G);
    mm_load_input(p, g, G, r0, nr);
    __syncthreads();
    mm_hidden(G, nr);
    const int l = G.geo.L - 1, win = G.geo.win[l], N = G.N, ldi = mm_ld(win);
    for (int i = threadIdx.x; i < nr * N; i += MM_THREADS) {
        const int r = i / N, n = i - r * N;
        const float v = mm_dot(G.act[l] + r * ldi, G.w[l] + n * ldi, win, 0.f) + G.b[l][n];
        if (p.out_mode == 0) p.y[(int64_t)(r0 + r) * p.y_r + (int64_t)g * p.y_g + n] = v;
        else p.ws[((int64_t)g * p.rows + r0 + r) * p.n_max + n] = v;
    }
}

// max-scatter: latent[r][j] = act(max over the owners (g, n) of j, in group order, of y_g[r][n]); the first of equal values
// wins (torch.max over dim 1 of the stacked spaces), a NaN wins over everything after it; no owner: -inf, winner -1
__global__ __launch_bounds__(256) void multi_mlp_scatter_kernel(as_multi_mlp p) {
    const int64_t total = (int64_t)p.rows * p.latent;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / p.latent), j = (int)(i - (int64_t)r * p.latent);
        float best = -INFINITY;
        int win = -1;
        for (int q = p.own_ptr[j]; q < p.own_ptr[j + 1]; ++q) {
            const int e = p.own[q], gg = e / p.n_max, n = e - gg * p.n_max;
            const float v = p.ws[((int64_t)gg * p.rows + r) * p.n_max + n];
            if (win < 0 || (!isnan(best) && (isnan(v) || v > best))) { best = v; win = e; }
        }
        p.y[(int64_t)r * p.y_r + j] = p.act ? tanhf(best) : best;
        p.win[i] = win;
    }
}

__global__ __launch_bounds__(MM_THREADS) void multi_mlp_bwd_kernel(as_multi_mlp p, int chunks, float* part, float* wsdx) {
    extern __shared__ float lds[];
    __shared__ MMGroup G;   // in LDS, not registers: the per-layer arrays are indexed by a loop variable
    __shared__ MMGeo gm;
    __shared__ float* dz[3];
    const int g = blockIdx.y, G_ = p.groups;
    if (threadIdx.x == 0) {
        mm_group(G, p, g, lds);
        gm = mm_geo(p.layers, p.k_max, p.n_max, p.h1, p.h2);
        float* s = G.act[0] + MM_RT * mm_act_floats(gm);
        for (int l = 0; l < gm.L; ++l) { dz[l] = s; s += MM_RT * mm_ld(gm.wout[l]); }
    }
    __syncthreads();
    const int64_t P = mm_slot_off(gm, gm.L);
    float* slot = part ? part + ((int64_t)blockIdx.x * G_ + g) * P : nullptr;
    mm_stage_weights(p, g, G);
    if (slot) {   // zero the tails of the slot that a narrower group does not fill (the chunk sum runs over the whole slot)
        for (int l = 0; l < gm.L; ++l) {
            float* w = slot + mm_slot_off(gm, l);
            const int used = G.geo.wout[l] * G.geo.win[l], all = gm.wout[l] * gm.win[l];
            for (int i = used + threadIdx.x; i < all; i += MM_THREADS) w[i] = 0.f;
            for (int i = G.geo.wout[l] + threadIdx.x; i < gm.wout[l]; i += MM_THREADS) w[all + i] = 0.f;
        }
    }
    const int tiles = (p.rows + MM_RT - 1) / MM_RT, L = G.geo.L, N = G.N;
    for (int t = blockIdx.x; t < tiles; t += chunks) {
        const bool first = t == (int)blockIdx.x;
        const int r0 = t * MM_RT, nr = min(MM_RT, p.rows - r0);
        __syncthreads();   // the previous tile's readers of act / dz are done
        mm_load_input(p, g, G, r0, nr);
        __syncthreads();
        mm_hidden(G, nr);
        // gradient of the last layer's output
        const int ldn = mm_ld(N);
        for (int i = threadIdx.x; i < nr * N; i += MM_THREADS) {
            const int r = i / N, n = i - r * N;
            const int64_t row = (int64_t)(r0 + r) * p.y_r;
            float d;
            if (p.out_mode == 0) {
                d = p.dy[row + (int64_t)g * p.y_g + n];
            } else {
                const int j = p.out_idx[g * p.n_max + n], e = g * p.n_max + n;
                d = 0.f;
                if ((unsigned)j < (unsigned)p.latent && p.win[(int64_t)(r0 + r) * p.latent + j] == e) {
                    d = p.dy[row + j];
                    if (p.act) {
                        const float yv = p.y[row + j];
                        d = d * (1.f - yv * yv);
                    }
                }
            }
            dz[L - 1][r * ldn + n] = d;
        }
        __syncthreads();
        for (int l = L - 1; l >= 0; --l) {
            const int win = G.geo.win[l], wout = G.geo.wout[l], ldi = mm_ld(win), ldo = mm_ld(wout);
            if (slot) {
                float* w = slot + mm_slot_off(gm, l);
                for (int i = threadIdx.x; i < wout * win; i += MM_THREADS) {
                    const int n = i / win, k = i - n * win;
                    float s = 0.f;
                    for (int r = 0; r < nr; ++r) s = fmaf(dz[l][r * ldo + n], G.act[l][r * ldi + k], s);
                    w[i] = first ? s : w[i] + s;
                }
                float* b = w + (int64_t)gm.wout[l] * gm.win[l];
                for (int n = threadIdx.x; n < wout; n += MM_THREADS) {
                    float s = 0.f;
                    for (int r = 0; r < nr; ++r) s += dz[l][r * ldo + n];
                    b[n] = first ? s : b[n] + s;
                }
            }
            if (l > 0) {   // through W_l and the ReLU of its input (torch: grad * (out > 0))
                for (int i = threadIdx.x; i < nr * win; i += MM_THREADS) {
                    const int r = i / win, k = i - r * win;
                    float s = 0.f;
                    for (int n = 0; n < wout; ++n) s = fmaf(dz[l][r * ldo + n], G.w[l][n * ldi + k], s);
                    dz[l - 1][r * ldi + k] = G.act[l][r * ldi + k] > 0.f ? s : 0.f;
                }
                __syncthreads();
            } else if (p.dx) {
                for (int i = threadIdx.x; i < nr * win; i += MM_THREADS) {
                    const int r = i / win, k = i - r * win;
                    float s = 0.f;
                    for (int n = 0; n < wout; ++n) s = fmaf(dz[0][r * ldo + n], G.w[0][n * ldi + k], s);
                    if (p.in_mode == 0) p.dx[(int64_t)(r0 + r) * p.x_r + (int64_t)g * p.x_g + k] = s;
                    else wsdx[((int64_t)g * p.rows + r0 + r) * p.k_max + k] = s;
                }
            }
        }
    }
}

// gather mode: dx[r][j] = in_scale * sum over the readers (g, k) of j, in group order, of dx_g[r][k]; 0 for an unread j
__global__ __launch_bounds__(256) void multi_mlp_gather_dx_kernel(as_multi_mlp p, const float* __restrict__ wsdx) {
    const int64_t total = (int64_t)p.rows * p.latent;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / p.latent), j = (int)(i - (int64_t)r * p.latent);
        float s = 0.f;
        for (int q = p.own_ptr[j]; q < p.own_ptr[j + 1]; ++q) {
            const int e = p.own[q], gg = e / p.k_max, k = e - gg * p.k_max;
            s += wsdx[((int64_t)gg * p.rows + r) * p.k_max + k];
        }
        p.dx[(int64_t)r * p.x_r + j] = s * p.in_scale;
    }
}

inline int mm_grid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

bool mm_fits(int32_t layers, int32_t k_max, int32_t h1, int32_t h2, int32_t n_max) {
    if (layers != 1 && layers != 3) return false;
    if (k_max < 1 || n_max < 1 || k_max > MM_MAX_WIDTH || n_max > MM_MAX_WIDTH) return false;
    if (layers == 3 && (h1 < 1 || h2 < 1 || h1 > MM_MAX_WIDTH || h2 > MM_MAX_WIDTH)) return false;
    return mm_lds_bytes(mm_geo(layers, k_max, n_max, h1, h2), true) <= MM_MAX_LDS;
}

int64_t mm_chunks(int32_t rows) { return std::min<int64_t>(MM_CHUNKS, (rows + MM_RT - 1) / MM_RT); }

int mm_check(const as_multi_mlp* p, const char* who) {
    AS_REQUIRE(p, AS_ERR_BAD_ARG, "%s: null descriptor", who);
    AS_REQUIRE(p->groups > 0 && p->rows > 0 && (p->layers == 1 || p->layers == 3), AS_ERR_BAD_ARG,
               "%s: groups=%d rows=%d layers=%d", who, p->groups, p->rows, p->layers);
    AS_REQUIRE(p->groups <= 65535, AS_ERR_BAD_ARG, "%s: %d groups", who, p->groups);
    AS_REQUIRE(mm_fits(p->layers, p->k_max, p->h1, p->h2, p->n_max), AS_ERR_UNSUPPORTED,
               "%s: widths K<=%d h=%d/%d N<=%d exceed the LDS budget (every width <= %d, %d KB per workgroup)", who, p->k_max,
               p->h1, p->h2, p->n_max, MM_MAX_WIDTH, MM_MAX_LDS / 1024);
    AS_REQUIRE(p->dims && p->params && p->x, AS_ERR_BAD_ARG, "%s: null dims / params / x", who);
    AS_REQUIRE(p->in_mode == 0 || p->in_mode == 1, AS_ERR_BAD_ARG, "%s: in_mode %d", who, p->in_mode);
    AS_REQUIRE(p->out_mode == 0 || p->out_mode == 1, AS_ERR_BAD_ARG, "%s: out_mode %d", who, p->out_mode);
    AS_REQUIRE(!(p->in_mode == 1 && p->out_mode == 1), AS_ERR_BAD_ARG, "%s: gather input with max-scatter output", who);
    if (p->in_mode == 1 || p->out_mode == 1) {
        AS_REQUIRE(p->latent > 0 && p->own_ptr && p->own, AS_ERR_BAD_ARG, "%s: latent=%d / null owner table", who, p->latent);
    }
    AS_REQUIRE(p->in_mode == 0 || p->in_idx, AS_ERR_BAD_ARG, "%s: gather input without in_idx", who);
    AS_REQUIRE(p->out_mode == 0 || (p->out_idx && p->win), AS_ERR_BAD_ARG, "%s: max-scatter without out_idx / win", who);
    AS_REQUIRE(p->act == 0 || p->act == 1, AS_ERR_BAD_ARG, "%s: act %d", who, p->act);
    return 0;
}

}  // namespace

extern "C" int32_t as_multi_mlp_supported(int32_t layers, int32_t k_max, int32_t h1, int32_t h2, int32_t n_max) {
    return mm_fits(layers, k_max, h1, h2, n_max) ? 1 : 0;
}

extern "C" int64_t as_multi_mlp_param_floats(int32_t layers, int32_t k_max, int32_t h1, int32_t h2, int32_t n_max) {
    if (layers != 1 && layers != 3) return -1;
    const MMGeo gm = mm_geo(layers, k_max, n_max, h1, h2);
    return mm_slot_off(gm, gm.L);
}

extern "C" int64_t as_multi_mlp_workspace_floats(const as_multi_mlp* p, int32_t backward) {
    if (!p || p->groups <= 0 || p->rows <= 0 || (p->layers != 1 && p->layers != 3)) return -1;
    if (!backward) return p->out_mode == 1 ? (int64_t)p->groups * p->rows * p->n_max : 0;
    int64_t n = 0;
    if (p->dparams) n += mm_chunks(p->rows) * p->groups * as_multi_mlp_param_floats(p->layers, p->k_max, p->h1, p->h2, p->n_max);
    if (p->dx && p->in_mode == 1) n += (int64_t)p->groups * p->rows * p->k_max;
    return n;
}

extern "C" int as_multi_mlp_fwd(const as_multi_mlp* p, void* stream) {
    AS_TRY(mm_check(p, "as_multi_mlp_fwd"));
    AS_REQUIRE(p->y, AS_ERR_BAD_ARG, "as_multi_mlp_fwd: null y");
    const int64_t need = as_multi_mlp_workspace_floats(p, 0);
    AS_REQUIRE(need == 0 || (p->ws && p->ws_floats >= need), AS_ERR_WORKSPACE, "as_multi_mlp_fwd: workspace %ld < %ld floats",
               (long)p->ws_floats, (long)need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t shm = mm_lds_bytes(mm_geo(p->layers, p->k_max, p->n_max, p->h1, p->h2), false);
    AS_REQUIRE(shm <= 64 * 1024 || as_allow_dynamic_lds(multi_mlp_fwd_kernel, MM_MAX_LDS) == hipSuccess, AS_ERR_UNSUPPORTED, "as_multi_mlp_fwd: %ld B of LDS refused",
               (long)shm);
    AS_PROF("multi_mlp_fwd", st);
    hipLaunchKernelGGL(multi_mlp_fwd_kernel, dim3((p->rows + MM_RT - 1) / MM_RT, p->groups), dim3(MM_THREADS), (size_t)shm, st, *p);
    AS_LAUNCH_CHECK("as_multi_mlp_fwd");
    if (p->out_mode == 1) {
        hipLaunchKernelGGL(multi_mlp_scatter_kernel, dim3(mm_grid((int64_t)p->rows * p->latent)), dim3(256), 0, st, *p);
        AS_LAUNCH_CHECK("as_multi_mlp_fwd (max-scatter)");
    }
    return 0;
}

extern "C" int as_multi_mlp_bwd(const as_multi_mlp* p, void* stream) {
    AS_TRY(mm_check(p, "as_multi_mlp_bwd"));
    AS_REQUIRE(p->dy && (p->dx || p->dparams), AS_ERR_BAD_ARG, "as_multi_mlp_bwd: needs dy and one of dx / dparams");
    AS_REQUIRE(p->out_mode == 0 || !p->act || p->y, AS_ERR_BAD_ARG, "as_multi_mlp_bwd: tanh max-scatter needs the forward's y");
    const int64_t need = as_multi_mlp_workspace_floats(p, 1);
    AS_REQUIRE(need == 0 || (p->ws && p->ws_floats >= need), AS_ERR_WORKSPACE, "as_multi_mlp_bwd: workspace %ld < %ld floats",
               (long)p->ws_floats, (long)need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t shm = mm_lds_bytes(mm_geo(p->layers, p->k_max, p->n_max, p->h1, p->h2), true);
    AS_REQUIRE(shm <= 64 * 1024 || as_allow_dynamic_lds(multi_mlp_bwd_kernel, MM_MAX_LDS) == hipSuccess, AS_ERR_UNSUPPORTED, "as_multi_mlp_bwd: %ld B of LDS refused",
               (long)shm);
    const int chunks = (int)mm_chunks(p->rows);
    const int64_t P = as_multi_mlp_param_floats(p->layers, p->k_max, p->h1, p->h2, p->n_max);
    float* part = p->dparams ? p->ws : nullptr;
    float* wsdx = (p->dx && p->in_mode == 1) ? p->ws + (p->dparams ? (int64_t)chunks * p->groups * P : 0) : nullptr;
    AS_PROF("multi_mlp_bwd", st);
    hipLaunchKernelGGL(multi_mlp_bwd_kernel, dim3(chunks, p->groups), dim3(MM_THREADS), (size_t)shm, st, *p, chunks, part, wsdx);
    AS_LAUNCH_CHECK("as_multi_mlp_bwd");
    if (wsdx) {
        hipLaunchKernelGGL(multi_mlp_gather_dx_kernel, dim3(mm_grid((int64_t)p->rows * p->latent)), dim3(256), 0, st, *p, wsdx);
        AS_LAUNCH_CHECK("as_multi_mlp_bwd (gather dx)");
    }
    if (part) AS_TRY(as_sum_partials(part, (long)p->groups * P, chunks, p->dparams, st));
    return 0;
}

// ---------------------------------------------------------------- fused masked / weighted MSE
namespace {
constexpr int MSE_BLOCKS = 1024;

__global__ __launch_bounds__(256) void masked_mse_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t rows,
                                                         int64_t feat, const int* __restrict__ lengths, int T,
                                                         const float* __restrict__ w, float scale, float* __restrict__ grad,
                                                         float* __restrict__ partial) {
    __shared__ float red[4];
    const int64_t n = rows * feat, stride = (int64_t)gridDim.x * 256;
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / feat;
        float wr = 1.f;
        if (lengths) wr = (int)(r % T) < lengths[r / T] ? 1.f : 0.f;
        if (w) wr *= w[r];
        const float d = a[i] - b[i];
        s += wr * (d * d);
        if (grad) grad[i] = 2.f * scale * wr * d;
    }
    s = as_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
}  // namespace

extern "C" int32_t as_masked_mse_partials(void) { return MSE_BLOCKS; }

extern "C" int as_masked_mse_fwd_bwd(const float* a, const float* b, int64_t rows, int64_t feat, const int32_t* lengths, int32_t T,
                                     const float* row_weights, float scale, float* loss, float* grad, float* partial, void* stream) {
    AS_REQUIRE(a && b && loss && partial, AS_ERR_BAD_ARG, "as_masked_mse_fwd_bwd: null pointer");
    AS_REQUIRE(rows > 0 && feat > 0, AS_ERR_BAD_ARG, "as_masked_mse_fwd_bwd: rows=%ld feat=%ld", (long)rows, (long)feat);
    AS_REQUIRE(!lengths || (T > 0 && rows % T == 0), AS_ERR_BAD_ARG, "as_masked_mse_fwd_bwd: rows=%ld not a multiple of T=%d",
               (long)rows, T);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = rows * feat;
    int blocks = (int)std::min<int64_t>((n + 255) / 256, MSE_BLOCKS);
    hipLaunchKernelGGL(masked_mse_kernel, dim3(blocks), dim3(256), 0, st, a, b, rows, feat, lengths, T, row_weights, scale, grad,
                       partial);
    AS_LAUNCH_CHECK("as_masked_mse_fwd_bwd");
    return as_loss_final(partial, blocks, scale, loss, st);
}
