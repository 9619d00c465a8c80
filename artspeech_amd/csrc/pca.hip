// Incremental PCA of the articulator contours (reference train_articulatory_PCA.py:91-108: one
// sklearn.decomposition.IncrementalPCA.partial_fit per loader batch and articulator), fitted on the device.
//
// The work splits like a GRU layer:
//   time-parallel   pca_batch_stats_kernel  per (batch, articulator): the batch mean and the centred sums of squares
//                   pca_cross_kernel        per (batch, articulator): the centred cross-products (X - xbar)^T (X - xbar), only
//                                           for the batches whose merge is solved on the feature side
//   sequential      pca_chain_kernel        one persistent workgroup per articulator walks its chain of batches in ONE launch:
//                                           mean / variance update (Chan), the merge, a symmetric eigen-solve by parallel-ordered
//                                           cyclic Jacobi, truncation to k, the sign rule
// Arithmetic: everything after the fp32 loads is fp64 (plain FMAs).  The merged matrix M of a step has the rows S V (k),
// X - xbar (m) and sqrt(n m / n') (mean - xbar) (1); its right singular vectors are the eigenvectors of M^T M (order F, "feature
// side", built from the cross-products) or, when M has fewer rows than columns, M^T U / s from the eigenvectors U of M M^T
// ("sample side").  In fp64 the squared condition number costs nothing that survives the rounding of the stored fp32 results.
// The chain state (mean, variance, singular values, components) lives in fp64 in the caller's state buffer, so a fit continued
// by a second call equals one call over all batches bit for bit.  No atomics: every sum has a fixed order.
#include <algorithm>

#include "as_common.h"
#include "as_launch.h"

#define PCA_MAX_F 256
#define PCA_MAX_K 64
#define PCA_LDS_ORDER 140     // largest (even-padded) matrix order whose matrix is kept in LDS (153 KB of fp64)
#define PCA_LDS_BOTH 100      // ... whose matrix AND eigenvector accumulator are (2 x 78 KB: F = 100 fits, with 3.2 KB of static LDS)
#define PCA_MAX_LDS (2 * PCA_LDS_BOTH * PCA_LDS_BOTH * 8)
#define PCA_MAX_SWEEPS 30     // cyclic Jacobi converges quadratically: ~6-10 sweeps in fp64; the loop never exceeds this
#define PCA_CT 64             // cross-product output tile

namespace {

struct PcaWs {
    double* bmean;   // [nb][A][F]
    double* bss;     // [nb][A][F]   sum (x - xbar)^2
    double* cross;   // [nb][A][F][F] or null
    double* G;       // [A][NE * NE]
    double* Qt;      // [A][NE * NE]
    double* M;       // [A][F * F]
    double* vec;     // [A][F]       the mean-correction row
    int32_t nb, ne;  // batches of this call; even-padded bound of the matrix order
};

__host__ __device__ inline int64_t pca_state_doubles(int F, int k_max) { return 2 * (int64_t)F + k_max + (int64_t)k_max * F; }

__device__ __forceinline__ int64_t pca_row(const as_pca& p, int64_t r) { return p.order ? (int64_t)p.order[r] : r; }

// rows of the merged matrix of batch j for an articulator with k components
__device__ __forceinline__ int pca_merge_rows(const as_pca& p, int j, int m, int k) { return (p.n_seen == 0 && j == 0) ? m : k + m + 1; }

__global__ __launch_bounds__(256) void pca_batch_stats_kernel(as_pca p, PcaWs w) {
    const int j = blockIdx.x, a = blockIdx.y, F = p.features;
    const int64_t r0 = (int64_t)j * p.batch;
    const int m = (int)min((int64_t)p.batch, p.rows - r0);
    double* bm = w.bmean + ((int64_t)j * p.groups + a) * F;
    double* bs = w.bss + ((int64_t)j * p.groups + a) * F;
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        const float* x = p.x + (int64_t)a * p.x_g + f;
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += (double)x[pca_row(p, r0 + i) * p.x_r];
        const double mean = s / m;
        double q = 0.0;
        for (int i = 0; i < m; ++i) {
            const double d = (double)x[pca_row(p, r0 + i) * p.x_r] - mean;
            q = fma(d, d, q);
        }
        bm[f] = mean;
        bs[f] = q;
    }
}

// C[p][q] = sum_i (x_ip - xbar_p)(x_iq - xbar_q): one 64 x 64 tile per workgroup, 4 x 4 per thread, rows in chunks of 16
__global__ __launch_bounds__(256) void pca_cross_kernel(as_pca p, PcaWs w) {
    __shared__ double sp[16][PCA_CT], sq[16][PCA_CT];
    const int F = p.features, tiles = (F + PCA_CT - 1) / PCA_CT;
    const int tile = blockIdx.x % (tiles * tiles), j = blockIdx.x / (tiles * tiles), a = blockIdx.y;
    const int tp = tile / tiles, tq = tile % tiles;
    const int64_t r0 = (int64_t)j * p.batch;
    const int m = (int)min((int64_t)p.batch, p.rows - r0);
    if (pca_merge_rows(p, j, m, p.k[a]) < F) return;   // solved on the sample side: no cross-products
    const double* bm = w.bmean + ((int64_t)j * p.groups + a) * F;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4] = {};
    for (int i0 = 0; i0 < m; i0 += 16) {
        for (int e = threadIdx.x; e < 16 * PCA_CT; e += 256) {
            const int rr = e / PCA_CT, c = e % PCA_CT, i = i0 + rr;
            double vp = 0.0, vq = 0.0;
            if (i < m) {
                const float* x = p.x + pca_row(p, r0 + i) * p.x_r + (int64_t)a * p.x_g;
                const int fp = tp * PCA_CT + c, fq = tq * PCA_CT + c;
                if (fp < F) vp = (double)x[fp] - bm[fp];
                if (fq < F) vq = (double)x[fq] - bm[fq];
            }
            sp[rr][c] = vp;
            sq[rr][c] = vq;
        }
        __syncthreads();
#pragma unroll 4
        for (int rr = 0; rr < 16; ++rr) {
            double av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { av[u] = sp[rr][ty + 16 * u]; bv[u] = sq[rr][tx + 16 * u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(av[u], bv[v], acc[u][v]);
        }
        __syncthreads();
    }
    double* C = w.cross + ((int64_t)j * p.groups + a) * F * F;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int fp = tp * PCA_CT + ty + 16 * u, fq = tq * PCA_CT + tx + 16 * v;
            if (fp < F && fq < F) C[(int64_t)fp * F + fq] = acc[u][v];
        }
}

// maximum over the workgroup (independent of the order and of the workgroup's size); every thread gets the result
__device__ __forceinline__ double pca_block_max(double v, double* red) {
    v = as_wave_max_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) s = fmax(s, red[i]);
    return s;
}

// pair i of round rd of the round-robin tournament over ne (even) players
__device__ __forceinline__ void pca_pair(int ne, int rd, int i, int& p, int& q) {
    const int md = ne - 1;
    int x = (i == 0) ? md : (rd + i) % md;
    int y = (i == 0) ? rd : (rd - i + md) % md;
    p = min(x, y);
    q = max(x, y);
}

// MODE 0: matrix and eigenvector accumulator in (L2-resident) global memory; 1: matrix in LDS; 2: both in LDS
template <int MODE>
__global__ __launch_bounds__(1024) void pca_chain_kernel(as_pca p, PcaWs w) {
    extern __shared__ double s_dyn[];
    // static LDS is kept to 3.2 KB so that two matrices of order 100 fit beside it: the rotation table of the solve and the
    // eigenvalue table after it share their storage
    __shared__ double s_a[PCA_MAX_F + 2], s_red[16];
    __shared__ int s_i[PCA_MAX_F + 2];
    double* const s_cs = s_a;    // [2 * pairs] (c, s) of the round's rotations
    double* const s_lam = s_a;   // [n] eigenvalues, after the solve
    int* const s_pq = s_i;       // [pairs] p | q << 16
    int* const s_perm = s_i;     // [n] eigenvalue order, after the solve
    const int a = blockIdx.x, tid = threadIdx.x, T = blockDim.x, F = p.features, k = p.k[a], LD = w.ne;
    const int lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
    double* st = p.state + (int64_t)a * pca_state_doubles(F, p.k_max);
    double* sv_g = st + 2 * F;
    double* V_g = sv_g + p.k_max;   // [k_max][F]
    double* G = MODE >= 1 ? s_dyn : w.G + (int64_t)a * LD * LD;
    double* Qt = MODE == 2 ? s_dyn + LD * LD : w.Qt + (int64_t)a * LD * LD;
    double* M = w.M + (int64_t)a * F * F;
    double* cvec = w.vec + (int64_t)a * F;

    double n_seen = (double)p.n_seen;
    for (int j = 0; j < w.nb; ++j) {
        const int64_t r0 = (int64_t)j * p.batch;
        const int m = (int)min((int64_t)p.batch, p.rows - r0);
        const bool first = (p.n_seen == 0 && j == 0);
        const double nn = n_seen + m;
        const double* bm = w.bmean + ((int64_t)j * p.groups + a) * F;
        const double* bs = w.bss + ((int64_t)j * p.groups + a) * F;
        const int r = first ? m : k + m + 1;
        const bool small = r < F;
        const int n = small ? r : F;

        // ---- statistics (Chan) and the mean-correction row
        for (int f = tid; f < F; f += T) {
            const double b = bm[f];
            if (first) {
                cvec[f] = 0.0;
                st[f] = b;
                st[F + f] = bs[f] / nn;
            } else {
                const double mean = st[f], delta = b - mean, wgt = n_seen * m / nn;
                const double m2 = st[F + f] * n_seen + bs[f] + delta * delta * wgt;
                cvec[f] = -sqrt(wgt) * delta;
                st[f] = mean + delta * (m / nn);
                st[F + f] = m2 / nn;
            }
        }
        __syncthreads();

        // ---- the symmetric matrix of order n
        if (!small) {
            const double* C = w.cross + ((int64_t)j * p.groups + a) * F * F;
            for (int e = tid; e < F * F; e += T) {
                const int pp = e / F, qq = e % F;
                double g = C[e];
                if (!first) {
                    g = fma(cvec[pp], cvec[qq], g);
                    for (int i = 0; i < k; ++i) g = fma(sv_g[i] * sv_g[i] * V_g[i * F + pp], V_g[i * F + qq], g);
                }
                G[pp * LD + qq] = g;
            }
        } else {
            for (int e = tid; e < n * F; e += T) {
                const int t = e / F, f = e % F;
                double v;
                if (first) {
                    v = (double)p.x[pca_row(p, r0 + t) * p.x_r + (int64_t)a * p.x_g + f] - bm[f];
                } else if (t < k) {
                    v = sv_g[t] * V_g[t * F + f];
                } else if (t < k + m) {
                    v = (double)p.x[pca_row(p, r0 + t - k) * p.x_r + (int64_t)a * p.x_g + f] - bm[f];
                } else {
                    v = cvec[f];
                }
                M[e] = v;
            }
            __syncthreads();
            for (int e = tid; e < n * n; e += T) {
                const int pp = e / n, qq = e % n;
                const double* mp = M + (int64_t)pp * F;
                const double* mq = M + (int64_t)qq * F;
                double g = 0.0;
                for (int f = 0; f < F; ++f) g = fma(mp[f], mq[f], g);
                G[pp * LD + qq] = g;
            }
        }
        for (int e = tid; e < n * n; e += T) {
            const int pp = e / n, qq = e % n;
            Qt[pp * LD + qq] = pp == qq ? 1.0 : 0.0;
        }
        __syncthreads();

        // ---- parallel-ordered cyclic Jacobi: G <- J^T G J, Qt <- J^T Qt, n / 2 disjoint rotations per round
        const int ne = n + (n & 1), npairs = ne / 2;
        // element e = tid, tid + T, ... of an [npairs][n] / [n][npairs] walk without a division per element
        const int r_i0 = tid / n, r_c0 = tid % n, r_di = T / n, r_dc = T % n;
        const int c_r0 = tid / npairs, c_i0 = tid % npairs, c_dr = T / npairs, c_di = T % npairs;
        for (int sweep = 0; sweep < PCA_MAX_SWEEPS; ++sweep) {
            double off = 0.0, diag = 0.0;
            for (int pp = r_i0, qq = r_c0; pp < n;) {
                const double g = fabs(G[pp * LD + qq]);
                if (pp == qq) diag = fmax(diag, g); else off = fmax(off, g);
                qq += r_dc; pp += r_di;
                if (qq >= n) { qq -= n; ++pp; }
            }
            off = pca_block_max(off, s_red);
            diag = pca_block_max(diag, s_red);
            if (!(off > 1e-14 * diag)) break;   // uniform: every thread holds the same maxima
            for (int rd = 0; rd < ne - 1; ++rd) {
                if (tid < npairs) {
                    int pp, qq;
                    pca_pair(ne, rd, tid, pp, qq);
                    double c = 1.0, s = 0.0;
                    if (qq < n) {
                        const double apq = G[pp * LD + qq];
                        if (apq != 0.0) {
                            const double theta = (G[qq * LD + qq] - G[pp * LD + pp]) / (2.0 * apq);
                            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
                            c = 1.0 / sqrt(fma(t, t, 1.0));
                            s = t * c;
                        }
                    }
                    s_pq[tid] = pp | (qq << 16);
                    s_cs[2 * tid] = c;
                    s_cs[2 * tid + 1] = s;
                }
                __syncthreads();
                for (int i = r_i0, col = r_c0; i < npairs;) {   // rows of G and of Qt (the eigenvectors)
                    const double s = s_cs[2 * i + 1];
                    if (s != 0.0) {
                        const double c = s_cs[2 * i];
                        const int pp = s_pq[i] & 0xffff, qq = s_pq[i] >> 16;
                        const double gp = G[pp * LD + col], gq = G[qq * LD + col];
                        const double vp = Qt[pp * LD + col], vq = Qt[qq * LD + col];
                        G[pp * LD + col] = c * gp - s * gq;
                        G[qq * LD + col] = s * gp + c * gq;
                        Qt[pp * LD + col] = c * vp - s * vq;
                        Qt[qq * LD + col] = s * vp + c * vq;
                    }
                    col += r_dc; i += r_di;
                    if (col >= n) { col -= n; ++i; }
                }
                __syncthreads();
                for (int row = c_r0, i = c_i0; row < n;) {   // columns of G (consecutive threads: consecutive pairs)
                    const double s = s_cs[2 * i + 1];
                    if (s != 0.0) {
                        const double c = s_cs[2 * i];
                        const int pp = s_pq[i] & 0xffff, qq = s_pq[i] >> 16;
                        const double gp = G[row * LD + pp], gq = G[row * LD + qq];
                        G[row * LD + pp] = c * gp - s * gq;
                        G[row * LD + qq] = s * gp + c * gq;
                    }
                    i += c_di; row += c_dr;
                    if (i >= npairs) { i -= npairs; ++row; }
                }
                __syncthreads();
            }
        }

        // ---- eigenvalues, descending
        for (int i = tid; i < n; i += T) s_lam[i] = fmax(G[i * LD + i], 0.0);
        __syncthreads();
        for (int i = tid; i < n; i += T) {
            const double li = s_lam[i];
            int rank = 0;
            for (int t = 0; t < n; ++t) {
                const double lt = s_lam[t];
                rank += (lt > li || (lt == li && t < i)) ? 1 : 0;
            }
            s_perm[rank] = i;
        }
        __syncthreads();

        // ---- the k leading right singular vectors, one wave per component; largest-magnitude entry positive
        for (int i = wave; i < k; i += nwaves) {
            const int e = s_perm[i];
            const double lam = s_lam[e], s = sqrt(lam);
            double v[PCA_MAX_F / 64];
            double best = -1.0, best_v = 0.0;
            int best_f = 0;
#pragma unroll
            for (int u = 0; u < PCA_MAX_F / 64; ++u) {
                const int f = lane + 64 * u;
                double x = 0.0;
                if (f < F) {
                    if (!small) {
                        x = Qt[e * LD + f];
                    } else {
                        for (int t = 0; t < n; ++t) x = fma(Qt[e * LD + t], M[(int64_t)t * F + f], x);
                        x = s > 0.0 ? x / s : 0.0;
                    }
                    if (fabs(x) > best) { best = fabs(x); best_f = f; best_v = x; }
                }
                v[u] = x;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64), ov = __shfl_xor(best_v, o, 64);
                const int of = __shfl_xor(best_f, o, 64);
                if (ob > best || (ob == best && of < best_f)) { best = ob; best_f = of; best_v = ov; }
            }
            const double sign = best_v < 0.0 ? -1.0 : 1.0;
#pragma unroll
            for (int u = 0; u < PCA_MAX_F / 64; ++u) {
                const int f = lane + 64 * u;
                if (f < F) {
                    const double x = sign * v[u];
                    V_g[i * F + f] = x;
                    p.components[((int64_t)a * p.k_max + i) * F + f] = (float)x;
                }
            }
            if (lane == 0) {
                const int64_t o = (int64_t)a * p.k_max + i;
                sv_g[i] = s;
                p.singular_values[o] = (float)s;
                p.explained_variance[o] = (float)(lam / (nn - 1.0));
            }
        }
        if (wave == 0) {   // the scalars that need a sum: total variance, discarded variance
            double tot = 0.0, disc = 0.0;
            for (int f = lane; f < F; f += 64) tot += st[F + f] * nn;
            for (int i = k + lane; i < n; i += 64) disc += s_lam[s_perm[i]];
            tot = as_wave_sum_d(tot);
            disc = as_wave_sum_d(disc);
            for (int i = lane; i < k; i += 64)
                p.explained_variance_ratio[(int64_t)a * p.k_max + i] = (float)(s_lam[s_perm[i]] / tot);
            if (lane == 0)
                p.noise_variance[a] = (k == m || k == F || n <= k) ? 0.f : (float)(disc / (n - k) / (nn - 1.0));
        }
        n_seen = nn;
        __syncthreads();   // the new components are visible to the next step's build
    }
}

struct PcaPlan {
    int64_t nb, cslots, ne, doubles;
};

bool pca_plan(const as_pca* p, PcaPlan* pl) {
    if (!p || p->groups <= 0 || p->rows <= 0 || p->batch <= 0 || !as_pca_supported(p->features, p->k_max)) return false;
    const int64_t F = p->features;
    pl->nb = (p->rows + p->batch - 1) / p->batch;
    const int64_t order = std::min<int64_t>(F, (int64_t)p->k_max + p->batch + 1);
    pl->ne = order + (order & 1);
    pl->cslots = ((int64_t)p->k_max + std::min<int64_t>(p->batch, p->rows) + 1 >= F) ? pl->nb * p->groups : 0;
    pl->doubles = 2 * pl->nb * p->groups * F + pl->cslots * F * F + (int64_t)p->groups * (2 * pl->ne * pl->ne + F * F + F);
    return true;
}

}  // namespace

extern "C" int32_t as_pca_supported(int32_t features, int32_t k_max) {
    return (features >= 1 && features <= PCA_MAX_F && k_max >= 1 && k_max <= PCA_MAX_K && k_max <= features) ? 1 : 0;
}

extern "C" int64_t as_pca_workspace_floats(const as_pca* p) {
    PcaPlan pl;
    return pca_plan(p, &pl) ? 2 * pl.doubles : -1;
}

extern "C" int as_pca_fit(const as_pca* p, void* stream) {
    AS_REQUIRE(p, AS_ERR_BAD_ARG, "as_pca_fit: null descriptor");
    AS_REQUIRE(p->features >= 1 && p->k_max >= 1 && p->k_max <= p->features, AS_ERR_BAD_ARG,
               "as_pca_fit: n_components=%d must be in 1..features=%d", p->k_max, p->features);
    AS_REQUIRE(as_pca_supported(p->features, p->k_max), AS_ERR_UNSUPPORTED,
               "as_pca_fit: features=%d k_max=%d outside the kernel's limits (features <= %d, k <= min(features, %d))", p->features,
               p->k_max, PCA_MAX_F, PCA_MAX_K);
    AS_REQUIRE(p->groups > 0 && p->rows > 0 && p->batch > 0 && p->n_seen >= 0, AS_ERR_BAD_ARG,
               "as_pca_fit: groups=%d rows=%ld batch=%d n_seen=%ld", p->groups, (long)p->rows, p->batch, (long)p->n_seen);
    AS_REQUIRE(p->groups <= 65535 && p->rows < ((int64_t)1 << 40), AS_ERR_BAD_ARG, "as_pca_fit: groups=%d rows=%ld too large",
               p->groups, (long)p->rows);
    AS_REQUIRE(p->k && p->x && p->state && p->components && p->singular_values && p->explained_variance &&
                   p->explained_variance_ratio && p->noise_variance && p->ws,
               AS_ERR_BAD_ARG, "as_pca_fit: null pointer");
    AS_REQUIRE(p->n_seen > 0 || std::min<int64_t>(p->batch, p->rows) >= p->k_max, AS_ERR_BAD_ARG,
               "as_pca_fit: the first batch (%ld rows) must hold at least n_components=%d rows",
               (long)std::min<int64_t>(p->batch, p->rows), p->k_max);
    PcaPlan pl;
    AS_REQUIRE(pca_plan(p, &pl), AS_ERR_BAD_ARG, "as_pca_fit: bad descriptor");
    AS_REQUIRE(pl.nb <= (1 << 26), AS_ERR_BAD_ARG, "as_pca_fit: %ld batches in one call", (long)pl.nb);
    AS_REQUIRE(p->ws_floats >= 2 * pl.doubles, AS_ERR_WORKSPACE, "as_pca_fit: workspace of %ld floats, %ld needed", (long)p->ws_floats,
               (long)(2 * pl.doubles));
    AS_REQUIRE(((uintptr_t)p->ws & 7) == 0 && ((uintptr_t)p->state & 7) == 0, AS_ERR_BAD_ARG, "as_pca_fit: ws / state not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t F = p->features, A = p->groups;
    PcaWs w;
    double* base = reinterpret_cast<double*>(p->ws);
    w.bmean = base;
    w.bss = w.bmean + pl.nb * A * F;
    w.cross = pl.cslots ? w.bss + pl.nb * A * F : nullptr;
    w.G = w.bss + pl.nb * A * F + pl.cslots * F * F;
    w.Qt = w.G + A * pl.ne * pl.ne;
    w.M = w.Qt + A * pl.ne * pl.ne;
    w.vec = w.M + A * F * F;
    w.nb = (int32_t)pl.nb;
    w.ne = (int32_t)pl.ne;
    {
        AS_PROF("pca_batch_stats", st);
        hipLaunchKernelGGL(pca_batch_stats_kernel, dim3((unsigned)pl.nb, (unsigned)A), dim3(256), 0, st, *p, w);
        AS_LAUNCH_CHECK("as_pca_fit (batch statistics)");
        if (pl.cslots) {
            const int tiles = (int)((F + PCA_CT - 1) / PCA_CT);
            hipLaunchKernelGGL(pca_cross_kernel, dim3((unsigned)(tiles * tiles * pl.nb), (unsigned)A), dim3(256), 0, st, *p, w);
            AS_LAUNCH_CHECK("as_pca_fit (cross-products)");
        }
    }
    // where the matrix and the eigenvector accumulator live changes no arithmetic: a refused LDS size falls back to the next mode
    int mode = pl.ne <= PCA_LDS_BOTH ? 2 : (pl.ne <= PCA_LDS_ORDER ? 1 : 0);
    const size_t one = (size_t)pl.ne * pl.ne * 8;
    if (mode == 2 && 2 * one > 64 * 1024 && as_allow_dynamic_lds(pca_chain_kernel<2>, PCA_MAX_LDS) != hipSuccess) mode = 1;
    if (mode == 1 && one > 64 * 1024 && as_allow_dynamic_lds(pca_chain_kernel<1>, PCA_MAX_LDS) != hipSuccess) mode = 0;
    const int threads = pl.ne <= 48 ? 256 : 1024;
    AS_PROF("pca_chain", st);
    if (mode == 2)
        hipLaunchKernelGGL(pca_chain_kernel<2>, dim3((unsigned)A), dim3(threads), 2 * one, st, *p, w);
    else if (mode == 1)
        hipLaunchKernelGGL(pca_chain_kernel<1>, dim3((unsigned)A), dim3(threads), one, st, *p, w);
    else
        hipLaunchKernelGGL(pca_chain_kernel<0>, dim3((unsigned)A), dim3(threads), 0, st, *p, w);
    AS_LAUNCH_CHECK("as_pca_fit (chain)");
    return 0;
}
