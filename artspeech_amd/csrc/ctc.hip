// CTC loss (torch.nn.CTCLoss, as phoneme_recognition/__init__.py:114-120 calls it) over strided (T, B, C) rows:
//   ctc_row_lse_kernel     : logits mode only -- lse[b][t] = logsumexp_c x[t][b][c], one wave per row (fixed butterfly), so the
//                            recursions read log-probabilities x - lse without a separate log-softmax pass.
//   ctc_alpha_beta_kernel  : the forward (alpha) and backward (beta) log-space recursions of one utterance, concurrently:
//                            blockIdx.y = 0 runs alpha over t = 0 .. Tb-1, blockIdx.y = 1 runs beta over t = Tb-1 .. 0.  Beta is
//                            alpha over reversed time and the reversed extended label sequence (blank, l_L, blank, ..., l_1,
//                            blank is again an extended sequence), so one code path serves both: thread k holds the SPT
//                            consecutive (reversed for beta) states k*SPT .. k*SPT+SPT-1 in registers, and each step needs only
//                            the previous thread's last two states -- cross-lane shifts inside one wave (S <= 256, the common
//                            case: collapsed phoneme targets), an LDS exchange with one barrier per step (double-buffered)
//                            beyond that (S <= 4095).  Every step's values go to the workspace for the gradient pass;
//                            alpha's last step gives nll[b].
//   ctc_grad_kernel        : one wave per (t, b): grad[t][b][k] = (exp(lp) - exp(lcab_k + nll - lp)) * scale[b] with
//                            lcab_k = logsumexp over the states s with l'_s = k of alpha_t(s) + beta_t(s) (torch's own formula,
//                            LossCTC.cpp), each class summed by one lane in state order: deterministic.  Rows t >= Tb and,
//                            with zero_infinity, utterances whose nll is infinite get zeros.
#include <math.h>

#include "as_common.h"
#include "ctc_common.h"

namespace {

__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + logf(expf(a - m) + expf(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

__global__ __launch_bounds__(256) void ctc_row_lse_kernel(const float* __restrict__ x, long sxt, long sxb, int T, int B, int C,
                                                          float* __restrict__ lse) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // row = b * T + t
    const int lane = threadIdx.x & 63;
    if (row >= (long)B * T) return;   // wave-uniform
    const int b = (int)(row / T), t = (int)(row % T);
    const float* xr = x + t * sxt + b * sxb;
    float m = -INFINITY;
    for (int k = lane; k < C; k += 64) m = fmaxf(m, xr[k]);
    m = as_wave_max(m);
    float s = 0.f;
    if (m != -INFINITY)
        for (int k = lane; k < C; k += 64) s += expf(xr[k] - m);
    s = as_wave_sum(s);
    if (lane == 0) lse[row] = m == -INFINITY ? -INFINITY : m + logf(s);
}

template <int NT, int SPT>
__global__ __launch_bounds__(NT) void ctc_alpha_beta_kernel(const float* __restrict__ x, long sxt, long sxb, int T, const float* __restrict__ lse,
                                                            const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                            const int64_t* __restrict__ in_len, const int64_t* __restrict__ tgt_len, int maxL,
                                                            int blank, float* __restrict__ alpha, float* __restrict__ beta,
                                                            float* __restrict__ nll) {
    __shared__ float xch[2][NT][2];
    __shared__ float fin[2];
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    int L = 0, Tb = 0;
    long toff = 0;
    if (!ctc_sizes(in_len, tgt_len, targets, tgt_stride, b, T, maxL, L, Tb, toff)) {   // block-uniform
        if (dir == 0 && tid == 0) nll[b] = NAN;
        return;
    }
    if (Tb == 0) {
        if (dir == 0 && tid == 0) nll[b] = L == 0 ? 0.f : INFINITY;
        return;
    }
    const int S = 2 * L + 1, Smax = 2 * maxL + 1;
    float* out = (dir ? beta : alpha) + (long)b * T * Smax;
    // per state: its label, whether the skip transition from r - 2 is allowed, its address in the workspace row
    int lab[SPT], sidx[SPT];
    bool skip[SPT], live[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int r = tid * SPT + i;
        live[i] = r < S;
        const int s = dir ? S - 1 - r : r;
        sidx[i] = s;
        lab[i] = (live[i] && (s & 1)) ? (int)targets[toff + (s >> 1)] : blank;
        skip[i] = false;
        if (live[i] && (r & 1) && r >= 2) {
            const int s2 = dir ? s + 2 : s - 2;   // state r - 2 in this direction
            skip[i] = lab[i] != (int)targets[toff + (s2 >> 1)];
        }
    }
    float a[SPT];
    for (int tau = 0; tau < Tb; ++tau) {
        const int t = dir ? Tb - 1 - tau : tau;
        const float* row = x + t * sxt + (long)b * sxb;
        const float sub = lse ? lse[(long)b * T + t] : 0.f;
        float lp[SPT];
#pragma unroll
        for (int i = 0; i < SPT; ++i) lp[i] = live[i] ? row[lab[i]] - sub : -INFINITY;
        if (tau == 0) {
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int r = tid * SPT + i;
                a[i] = (live[i] && r < 2) ? lp[i] : -INFINITY;
            }
        } else {
            float p1, p2;   // the previous thread's states r - 1 and r - 2 of its first state
            if constexpr (NT == 64) {
                p1 = __shfl_up(a[SPT - 1], 1, 64);
                p2 = __shfl_up(a[SPT - 2], 1, 64);
                if (tid == 0) p1 = p2 = -INFINITY;
            } else {
                const int par = tau & 1;
                xch[par][tid][0] = a[SPT - 1];
                xch[par][tid][1] = a[SPT - 2];
                __syncthreads();
                p1 = tid ? xch[par][tid - 1][0] : -INFINITY;
                p2 = tid ? xch[par][tid - 1][1] : -INFINITY;
            }
            float na[SPT];
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const float m1 = i >= 1 ? a[i - 1] : p1;
                const float m2 = i >= 2 ? a[i - 2] : (i == 1 ? p1 : p2);
                const float v = skip[i] ? lse3(a[i], m1, m2) : lse2(a[i], m1);
                na[i] = live[i] ? v + lp[i] : -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < SPT; ++i) a[i] = na[i];
        }
#pragma unroll
        for (int i = 0; i < SPT; ++i)
            if (live[i]) out[(long)t * Smax + sidx[i]] = a[i];
    }
    if (dir == 0) {
#pragma unroll
        for (int i = 0; i < SPT; ++i) {
            const int r = tid * SPT + i;
            if (r == S - 1) fin[0] = a[i];
            if (r == S - 2) fin[1] = a[i];
        }
        __syncthreads();
        if (tid == 0) nll[b] = -(S >= 2 ? lse2(fin[0], fin[1]) : fin[0]);
    }
}

__global__ __launch_bounds__(64) void ctc_grad_kernel(const float* __restrict__ x, long sxt, long sxb, int T, int C, const float* __restrict__ lse,
                                                      const int64_t* __restrict__ targets, int64_t tgt_stride, const int64_t* __restrict__ in_len,
                                                      const int64_t* __restrict__ tgt_len, int maxL, int blank, const float* __restrict__ alpha,
                                                      const float* __restrict__ beta, const float* __restrict__ nll,
                                                      const float* __restrict__ scale, int zero_inf, float* __restrict__ grad, long sgt,
                                                      long sgb) {
    __shared__ float lcab[2 * CTC_MAX_L + 1];
    __shared__ int labs[CTC_MAX_L];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    float* g = grad + t * sgt + (long)b * sgb;
    int L = 0, Tb = 0;
    long toff = 0;
    if (!ctc_sizes(in_len, tgt_len, targets, tgt_stride, b, T, maxL, L, Tb, toff)) {
        for (int k = lane; k < C; k += 64) g[k] = NAN;
        return;
    }
    const float nl = nll[b];
    if (t >= Tb || (zero_inf && isinf(nl))) {
        for (int k = lane; k < C; k += 64) g[k] = 0.f;
        return;
    }
    const int S = 2 * L + 1, Smax = 2 * maxL + 1;
    const float* ar = alpha + ((long)b * T + t) * Smax;
    const float* br = beta + ((long)b * T + t) * Smax;
    for (int j = lane; j < L; j += 64) labs[j] = (int)targets[toff + j];
    for (int s = lane; s < S; s += 64) lcab[s] = ar[s] + br[s];
    __syncthreads();
    const float* row = x + t * sxt + (long)b * sxb;
    const float sub = lse ? lse[(long)b * T + t] : 0.f;
    const float sc = scale ? scale[b] : 1.f;
    for (int k = lane; k < C; k += 64) {
        float m = -INFINITY;
        if (k == blank)
            for (int s = 0; s < S; s += 2) m = fmaxf(m, lcab[s]);
        for (int j = 0; j < L; ++j)
            if (labs[j] == k) m = fmaxf(m, lcab[2 * j + 1]);
        float lc = -INFINITY;
        if (m != -INFINITY) {
            float acc = 0.f;
            if (k == blank)
                for (int s = 0; s < S; s += 2) acc += expf(lcab[s] - m);
            for (int j = 0; j < L; ++j)
                if (labs[j] == k) acc += expf(lcab[2 * j + 1] - m);
            lc = m + logf(acc);
        }
        const float lp = row[k] - sub;
        g[k] = (expf(lp) - expf(lc + nl - lp)) * sc;
    }
}

}  // namespace

extern "C" int64_t as_ctc_workspace_floats(int32_t T, int32_t B, int32_t max_target_length) {
    if (T <= 0 || B <= 0 || max_target_length < 0) return 0;
    return (long)B * T + 2L * B * T * (2L * max_target_length + 1);
}

// the shared check, then the workspace that the loss fills and the gradient reads
static int ctc_check_ws(const char* who, const float* x, int32_t T, int32_t B, int32_t C, const int64_t* targets, const int64_t* in_len,
                        const int64_t* tgt_len, int32_t maxL, int32_t blank, int64_t ws_floats, const float* ws) {
    AS_TRY(ctc_check(who, x, T, B, C, targets, in_len, tgt_len, maxL, blank, ws != nullptr));
    AS_REQUIRE(ws_floats >= as_ctc_workspace_floats(T, B, maxL), AS_ERR_WORKSPACE, "%s: workspace of %lld floats, %lld needed", who,
               (long long)ws_floats, (long long)as_ctc_workspace_floats(T, B, maxL));
    return 0;
}

extern "C" int as_ctc_loss(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, int32_t logits,
                           const int64_t* targets, int64_t tgt_stride, const int64_t* input_lengths, const int64_t* target_lengths,
                           int32_t max_target_length, int32_t blank, int32_t with_beta, float* ws, int64_t ws_floats, float* nll,
                           void* stream) {
    AS_TRY(ctc_check_ws("as_ctc_loss", x, T, B, C, targets, input_lengths, target_lengths, max_target_length, blank, ws_floats, ws));
    AS_REQUIRE(nll, AS_ERR_BAD_ARG, "as_ctc_loss: null output");
    hipStream_t st = (hipStream_t)stream;
    const long S = 2L * max_target_length + 1;
    float* lse = logits ? ws : nullptr;
    float* alpha = ws + (long)B * T;
    float* beta = alpha + (long)B * T * S;
    if (logits) {
        hipLaunchKernelGGL(ctc_row_lse_kernel, dim3(as_cdiv((long)B * T, 4)), dim3(256), 0, st, x, (long)sx_t, (long)sx_b, T, B, C, lse);
        AS_LAUNCH_CHECK("as_ctc_loss");
    }
    const dim3 grid(B, with_beta ? 2 : 1);
    ctc_layout(max_target_length, [&](auto nt, auto spt) {
        constexpr int NT = decltype(nt)::value, SPT = decltype(spt)::value;
        hipLaunchKernelGGL((ctc_alpha_beta_kernel<NT, SPT>), grid, dim3(NT), 0, st, x, (long)sx_t, (long)sx_b, T, lse, targets, tgt_stride,
                           input_lengths, target_lengths, max_target_length, blank, alpha, beta, nll);
    });
    AS_LAUNCH_CHECK("as_ctc_loss");
    return 0;
}

extern "C" int as_ctc_grad(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, int32_t logits,
                           const int64_t* targets, int64_t tgt_stride, const int64_t* input_lengths, const int64_t* target_lengths,
                           int32_t max_target_length, int32_t blank, const float* ws, int64_t ws_floats, const float* nll,
                           const float* scale, int32_t zero_infinity, float* grad, int64_t sg_t, int64_t sg_b, void* stream) {
    AS_TRY(ctc_check_ws("as_ctc_grad", x, T, B, C, targets, input_lengths, target_lengths, max_target_length, blank, ws_floats, ws));
    AS_REQUIRE(nll && grad, AS_ERR_BAD_ARG, "as_ctc_grad: null argument");
    const long S = 2L * max_target_length + 1;
    const float* lse = logits ? ws : nullptr;
    const float* alpha = ws + (long)B * T;
    const float* beta = alpha + (long)B * T * S;
    hipLaunchKernelGGL(ctc_grad_kernel, dim3(T, B), dim3(64), 0, (hipStream_t)stream, x, (long)sx_t, (long)sx_b, T, C, lse, targets,
                       tgt_stride, input_lengths, target_lengths, max_target_length, blank, alpha, beta, nll, scale, zero_infinity, grad,
                       (long)sg_t, (long)sg_b);
    AS_LAUNCH_CHECK("as_ctc_grad");
    return 0;
}
