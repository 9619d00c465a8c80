// Parameter gradients of the DeepSpeech2-style scorer (phoneme_recognition/deepspeech2.py:15-81, trained by
// train_phoneme_recognition.py) on the channels-last maps [B][T][D][32] of conv.hip.  Every reduction is split into at most
// WG_MAX_PARTS fixed chunks whose partial sums are added in chunk order by ordered_rowsum_kernel: no atomics, and two identical
// calls give bit-identical results.
//   conv3x3_c32_wgrad_kernel  : dw[tap][co][ci] = sum_p dy[p][co] x[p + shift(tap)][ci] (zero padding), dbias[co] = sum_p dy[p][co]
//                               -- an implicit GEMM with a 32 x 288 output and a reduction over every position p = (b, t, d).
//                               Each wave walks a contiguous run of positions two at a time on the f32 MFMA
//                               (v_mfma_f32_32x32x2_f32: A = dy rows, B = x rows at the tap's shift, one 128-byte line each),
//                               the nine taps' 32 x 32 accumulators held for the whole run; the workgroup's four waves are
//                               added through LDS in wave order, one tap at a time, into the workgroup's partial.
//   conv3x3_stem_wgrad_kernel : the stem's dw[tap][co][ci] (Cin <= 4) and dbias: the same walk with the MFMA's 32 columns
//                               indexing (tap, ci) pairs, 9 * Cin <= 32 in one instruction (Cin <= 3) or two; the planar input
//                               is read through the forward's strides.
//   ln_feat_gelu_param_grad_kernel : dgamma[d] = sum_{r,c} dz * xhat, dbeta[d] = sum_{r,c} dz of ResidualCNN's feature-axis
//                               LayerNorm + GELU, dz = dy * gelu'(LN(x)); mean / rstd recomputed per (r, c) column.  A workgroup
//                               takes a run of rows and a tile of <= 128 features; its (d, c) sums live in LDS, one owner each.
//   ln_rows_param_grad_kernel : dgamma = sum_r dz * xhat, dbeta = sum_r dz of a row LayerNorm from its saved xhat, one
//                               thread per column over a run of rows.
#include "as_common.h"
#include "as_device.h"

namespace {

constexpr int CO = 32;
constexpr int WG_MAX_PARTS = 256;   // partial rows of every split reduction
constexpr int LN_DT = 128;          // feature tile of ln_feat_gelu_param_grad_kernel

// out[j] = sum_{i < n} part[i][j] (i ascending inside each of 16 contiguous row groups, then the groups in order); j < m0 goes
// to out0[j], the rest to out1[j - m0]
__global__ __launch_bounds__(256) void ordered_rowsum_kernel(const float* __restrict__ part, int n, int m, int m0, float* __restrict__ out0,
                                                             float* __restrict__ out1) {
    __shared__ float red[16][17];
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int j = blockIdx.x * 16 + c;
    const int per = (n + 15) / 16, i0 = g * per, i1 = min(n, i0 + per);
    float s = 0.f;
    if (j < m)
        for (int i = i0; i < i1; ++i) s += part[(long)i * m + j];
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && j < m) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) v += red[k][c];
        if (j < m0) out0[j] = v;
        else out1[j - m0] = v;
    }
}

// the workgroup's four accumulators of a 32 x 32 tile, added in wave order; element (row i, column j) -> dst[i * ld + j]
// for j < ncols (i: output channel)
__device__ __forceinline__ void reduce_tile(float (*red)[1024], const f32x16& acc, int wave, int lane, float* __restrict__ dst,
                                            const int* __restrict__ colmap, int ncols) {
    const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + l31] = acc[r];
    __syncthreads();
    for (int e = threadIdx.x; e < 1024; e += 256) {
        const int j = e & 31;
        if (j < ncols) dst[colmap ? colmap[e] : e] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
    }
    __syncthreads();
}

__device__ __forceinline__ void reduce_bias(float (*red)[1024], float bsum, int wave, int lane, float* __restrict__ dst) {
    bsum += __shfl_xor(bsum, 32, 64);   // positions k = 0 and 1 of every pair
    if (lane < 32) red[wave][lane] = bsum;
    __syncthreads();
    if (threadIdx.x < 32) dst[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    __syncthreads();
}

// part[blk][9 * 1024 + 32]; wave w of block blk covers positions [(4 blk + w) chunk, + chunk), chunk even
__global__ __launch_bounds__(256) void conv3x3_c32_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                float* __restrict__ part, int B, int T, int D, long chunk) {
    __shared__ float red[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lh = lane >> 5;
    const long P = (long)B * T * D;
    const long p0 = ((long)blockIdx.x * 4 + wave) * chunk;
    const long p1 = min(P, p0 + chunk);
    f32x16 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tap][r] = 0.f;
    float bsum = 0.f;

    for (long p = p0; p < p1; p += 2) {
        const long q = p + lh;   // this lane's position (the MFMA's k index)
        const bool ok = q < p1;
        const long qq = ok ? q : 0;
        const int d = (int)(qq % D), t = (int)((qq / D) % T);
        float a = dy[qq * CO + l31];
        a = ok ? a : 0.f;
        bsum += a;
        float bv[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int kd = tap / 3 - 1, kt = tap % 3 - 1;
            const bool in = ok && d + kd >= 0 && d + kd < D && t + kt >= 0 && t + kt < T;
            const float v = x[(in ? qq + (long)kt * D + kd : 0L) * CO + l31];
            bv[tap] = in ? v : 0.f;
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[tap], acc[tap], 0, 0, 0);
    }
    float* dst = part + (long)blockIdx.x * (9 * 1024 + CO);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) reduce_tile(red, acc[tap], wave, lane, dst + tap * 1024, nullptr, 32);
    reduce_bias(red, bsum, wave, lane, dst + 9 * 1024);
}

// part[blk][9 * 32 * CIN + 32]; the MFMA's column j = tap * CIN + ci (NM instructions of 32 columns)
template <int CIN>
__global__ __launch_bounds__(256) void conv3x3_stem_wgrad_kernel(const float* __restrict__ x, long sb, long sc, long sd, long st,
                                                                 const float* __restrict__ dy, float* __restrict__ part, int B, int T, int D,
                                                                 long chunk) {
    constexpr int NJ = 9 * CIN, NM = (NJ + 31) / 32;
    __shared__ float red[4][1024];
    __shared__ int colmap[NM][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lh = lane >> 5;
    for (int e = threadIdx.x; e < NM * 1024; e += 256) {   // tile element (co, j) -> dw[tap][co][ci]
        const int m = e >> 10, co = (e & 1023) >> 5, j = m * 32 + (e & 31);
        colmap[m][e & 1023] = j < NJ ? ((j / CIN) * CO + co) * CIN + j % CIN : 0;
    }
    const long P = (long)B * T * D;
    const long p0 = ((long)blockIdx.x * 4 + wave) * chunk;
    const long p1 = min(P, p0 + chunk);
    int jt[NM], jc[NM];
    bool jok[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        const int j = m * 32 + l31;
        jok[m] = j < NJ;
        jt[m] = jok[m] ? j / CIN : 0;
        jc[m] = jok[m] ? j % CIN : 0;
    }
    f32x16 acc[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    float bsum = 0.f;

    for (long p = p0; p < p1; p += 2) {
        const long q = p + lh;
        const bool ok = q < p1;
        const long qq = ok ? q : 0;
        const int d = (int)(qq % D), t = (int)((qq / D) % T);
        const long b = qq / ((long)D * T);
        float a = dy[qq * CO + l31];
        a = ok ? a : 0.f;
        bsum += a;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int kd = jt[m] / 3 - 1, kt = jt[m] % 3 - 1;
            const bool in = ok && jok[m] && d + kd >= 0 && d + kd < D && t + kt >= 0 && t + kt < T;
            const float v = x[in ? b * sb + jc[m] * sc + (long)(d + kd) * sd + (long)(t + kt) * st : 0L];
            acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, in ? v : 0.f, acc[m], 0, 0, 0);
        }
    }
    __syncthreads();   // colmap
    float* dst = part + (long)blockIdx.x * (9 * CO * CIN + CO);
#pragma unroll
    for (int m = 0; m < NM; ++m) reduce_tile(red, acc[m], wave, lane, dst, colmap[m], NJ - m * 32 < 32 ? NJ - m * 32 : 32);
    reduce_bias(red, bsum, wave, lane, dst + 9 * CO * CIN);
}

// part[blk][2][D] (gamma then beta); block (blk, feature tile ty) takes rows [blk * rows_per, +rows_per); 256 threads = 32 c x 8 d
__global__ __launch_bounds__(256) void ln_feat_gelu_param_grad_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, const float* __restrict__ dy, long R,
                                                                      int D, long rows_per, float eps, float* __restrict__ part) {
    __shared__ float accg[LN_DT][CO], accb[LN_DT][CO];
    __shared__ float red[8][CO];
    const int c = threadIdx.x & 31, dg = threadIdx.x >> 5;
    const int d0 = blockIdx.y * LN_DT, d1 = min(D, d0 + LN_DT);
    for (int d = d0 + dg; d < d1; d += 8) accg[d - d0][c] = accb[d - d0][c] = 0.f;
    const long r0 = (long)blockIdx.x * rows_per, r1 = min(R, r0 + rows_per);
    for (long r = r0; r < r1; ++r) {
        const float* xr = x + r * D * CO + c;
        const float* gr = dy + r * D * CO + c;
        float s = 0.f;
        for (int d = dg; d < D; d += 8) s += xr[d * CO];
        red[dg][c] = s;
        __syncthreads();
        float mean = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) mean += red[k][c];
        mean /= D;
        __syncthreads();
        float q = 0.f;
        for (int d = dg; d < D; d += 8) {
            const float e = xr[d * CO] - mean;
            q += e * e;
        }
        red[dg][c] = q;
        __syncthreads();
        float var = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) var += red[k][c];
        const float rs = 1.0f / sqrtf(var / D + eps);
        __syncthreads();
        for (int d = d0 + dg; d < d1; d += 8) {
            const float xh = (xr[d * CO] - mean) * rs;
            const float dz = gr[d * CO] * as_gelu_grad(xh * gamma[d] + beta[d]);
            accg[d - d0][c] += dz * xh;
            accb[d - d0][c] += dz;
        }
    }
    __syncthreads();
    float* dst = part + (long)blockIdx.x * 2 * D;
    for (int d = d0 + threadIdx.x; d < d1; d += 256) {
        float sg = 0.f, sbv = 0.f;
        for (int k = 0; k < CO; ++k) {
            sg += accg[d - d0][k];
            sbv += accb[d - d0][k];
        }
        dst[d] = sg;
        dst[D + d] = sbv;
    }
}

// part[blk][2][D]; block (blk, column tile) takes rows [blk * rows_per, +rows_per)
__global__ __launch_bounds__(256) void ln_rows_param_grad_kernel(const float* __restrict__ dz, const float* __restrict__ xhat, long R, int D,
                                                                 long rows_per, float* __restrict__ part) {
    const int d = blockIdx.y * 256 + threadIdx.x;
    if (d >= D) return;
    const long r0 = (long)blockIdx.x * rows_per, r1 = min(R, r0 + rows_per);
    float sg = 0.f, sbv = 0.f;
    for (long r = r0; r < r1; ++r) {
        const float g = dz[r * D + d];
        sg += g * xhat[r * D + d];
        sbv += g;
    }
    part[(long)blockIdx.x * 2 * D + d] = sg;
    part[(long)blockIdx.x * 2 * D + D + d] = sbv;
}

// positions per wave (even) and workgroups of a convolution's split
void conv_split(long P, long& chunk, int& blocks) {
    chunk = (P + 4L * WG_MAX_PARTS - 1) / (4L * WG_MAX_PARTS);
    chunk = (chunk + 1) & ~1L;
    if (chunk < 2) chunk = 2;
    blocks = (int)((P + 4 * chunk - 1) / (4 * chunk));
}

int ordered_rowsum(const float* part, int n, int m, int m0, float* out0, float* out1, hipStream_t st, const char* who) {
    hipLaunchKernelGGL(ordered_rowsum_kernel, dim3(as_cdiv(m, 16)), dim3(256), 0, st, part, n, m, m0, out0, out1);
    AS_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace

extern "C" int as_conv3x3_c32_wgrad(const float* x, const float* dy, float* dw, float* dbias, int32_t B, int32_t T, int32_t D, float* ws,
                                    int64_t ws_floats, void* stream) {
    AS_REQUIRE(x && dy && dw && dbias && ws && B > 0 && T > 0 && D > 0, AS_ERR_BAD_ARG, "as_conv3x3_c32_wgrad: bad argument");
    long chunk;
    int blocks;
    conv_split((long)B * T * D, chunk, blocks);
    const long need = (long)blocks * (9 * 1024 + CO);
    AS_REQUIRE(ws_floats >= need, AS_ERR_WORKSPACE, "as_conv3x3_c32_wgrad: workspace of %lld floats, %lld needed", (long long)ws_floats,
               (long long)need);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv3x3_c32_wgrad_kernel, dim3(blocks), dim3(256), 0, st, x, dy, ws, B, T, D, chunk);
    AS_LAUNCH_CHECK("as_conv3x3_c32_wgrad");
    return ordered_rowsum(ws, blocks, 9 * 1024 + CO, 9 * 1024, dw, dbias, st, "as_conv3x3_c32_wgrad");
}

extern "C" int as_conv3x3_stem_wgrad(const float* x, int64_t sb, int64_t sc, int64_t sd, int64_t st, const float* dy, float* dw,
                                     float* dbias, int32_t B, int32_t T, int32_t D, int32_t Cin, float* ws, int64_t ws_floats,
                                     void* stream) {
    AS_REQUIRE(x && dy && dw && dbias && ws && B > 0 && T > 0 && D > 0, AS_ERR_BAD_ARG, "as_conv3x3_stem_wgrad: bad argument");
    AS_REQUIRE(Cin >= 1 && Cin <= 4, AS_ERR_UNSUPPORTED, "as_conv3x3_stem_wgrad: %d input planes (1 to 4 supported)", Cin);
    long chunk;
    int blocks;
    conv_split((long)B * T * D, chunk, blocks);
    const int m = 9 * CO * Cin + CO;
    const long need = (long)blocks * m;
    AS_REQUIRE(ws_floats >= need, AS_ERR_WORKSPACE, "as_conv3x3_stem_wgrad: workspace of %lld floats, %lld needed", (long long)ws_floats,
               (long long)need);
    hipStream_t s = (hipStream_t)stream;
    as_up_to<1, 2, 3, 4>(Cin, [&](auto cin) {
        hipLaunchKernelGGL(conv3x3_stem_wgrad_kernel<decltype(cin)::value>, dim3(blocks), dim3(256), 0, s, x, (long)sb, (long)sc, (long)sd,
                           (long)st, dy, ws, B, T, D, chunk);
    });
    AS_LAUNCH_CHECK("as_conv3x3_stem_wgrad");
    return ordered_rowsum(ws, blocks, m, 9 * CO * Cin, dw, dbias, s, "as_conv3x3_stem_wgrad");
}

extern "C" int as_ln_feat_gelu_param_grad(const float* x, const float* gamma, const float* beta, const float* dy, int64_t rows, int32_t D,
                                          int32_t Cc, float* dgamma, float* dbeta, float* ws, int64_t ws_floats, void* stream) {
    AS_REQUIRE(x && gamma && beta && dy && dgamma && dbeta && ws && rows > 0 && D > 0, AS_ERR_BAD_ARG,
               "as_ln_feat_gelu_param_grad: bad argument");
    AS_REQUIRE(Cc == CO, AS_ERR_UNSUPPORTED, "as_ln_feat_gelu_param_grad: %d channels (32 supported)", Cc);
    const long rows_per = (rows + WG_MAX_PARTS - 1) / WG_MAX_PARTS;
    const int blocks = (int)((rows + rows_per - 1) / rows_per);
    const long need = (long)blocks * 2 * D;
    AS_REQUIRE(ws_floats >= need, AS_ERR_WORKSPACE, "as_ln_feat_gelu_param_grad: workspace of %lld floats, %lld needed",
               (long long)ws_floats, (long long)need);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ln_feat_gelu_param_grad_kernel, dim3(blocks, as_cdiv(D, LN_DT)), dim3(256), 0, st, x, gamma, beta, dy, (long)rows, D,
                       rows_per, 1e-5f, ws);
    AS_LAUNCH_CHECK("as_ln_feat_gelu_param_grad");
    return ordered_rowsum(ws, blocks, 2 * D, D, dgamma, dbeta, st, "as_ln_feat_gelu_param_grad");
}

extern "C" int as_layernorm_param_grad(const float* dz, const float* xhat, int64_t rows, int32_t D, float* dgamma, float* dbeta, float* ws,
                                       int64_t ws_floats, void* stream) {
    AS_REQUIRE(dz && xhat && dgamma && dbeta && ws && rows > 0 && D > 0, AS_ERR_BAD_ARG, "as_layernorm_param_grad: bad argument");
    const long rows_per = (rows + WG_MAX_PARTS - 1) / WG_MAX_PARTS;
    const int blocks = (int)((rows + rows_per - 1) / rows_per);
    const long need = (long)blocks * 2 * D;
    AS_REQUIRE(ws_floats >= need, AS_ERR_WORKSPACE, "as_layernorm_param_grad: workspace of %lld floats, %lld needed", (long long)ws_floats,
               (long long)need);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ln_rows_param_grad_kernel, dim3(blocks, as_cdiv(D, 256)), dim3(256), 0, st, dz, xhat, (long)rows, D, rows_per, ws);
    AS_LAUNCH_CHECK("as_layernorm_param_grad");
    return ordered_rowsum(ws, blocks, 2 * D, D, dgamma, dbeta, st, "as_layernorm_param_grad");
}
