// Frame-level phoneme classification on the device (reference phoneme_recognition/metrics.py: CrossEntropyLoss :87-120 and AUROC
// :185-197, the `loss: CE` branch of its scripts): the masked, class-weighted, label-smoothed cross-entropy with its gradient,
// and the one-vs-rest rank statistic behind the AUROC.  Rows are x[t*sx_t + b*sx_b + c] as in ctc.hip, one int64 target per frame.
//
//   as_frame_ce_loss   fc_loss_kernel: 16 lanes (one DPP row) per frame, the lanes across the classes -- the four rows of a wave
//                      are 4 * C consecutive floats of a (B, T, C) tensor, so the loads coalesce without staging.  Per frame in
//                      float32: the row maximum, sum exp(x - max), logsumexp, then the loss; the frames of a lane group are added
//                      in float64 in frame order, the 16 groups of a workgroup in group order, and the workgroups' partial sums
//                      (workspace) in workgroup order by whichever workgroup draws the last integer ticket.  The grid depends on
//                      (T, B) alone, so the order of every sum is fixed: no float atomics, repeats are bit-identical.  One launch.
//   as_frame_ce_grad   fc_grad_kernel: the same lane layout over ALL frames; p = exp(x - lse) from the saved logsumexp, the scale
//                      (gout, or gout / sum w[y]) read from device memory.  Every element of the gradient is written.
//   as_frame_auroc     fa_kernel: one workgroup of 1024 threads per class.  The valid frames' (order-preserving key of the score,
//                      positive flag) pairs are gathered into LDS as 64-bit words (an LDS integer counter hands out the slots:
//                      the order does not matter to a sort), sorted by a bitonic network, the low word is then replaced by the
//                      exclusive count of negatives in front of the entry, and every positive adds (negatives below its tie
//                      group) + (negatives up to and including its tie group): the group's start is found by bisection.
//                      At most 16384 frames (128 KiB of keys); integers throughout.
#include <math.h>

#include "as_common.h"
#include "as_device.h"
#include "as_launch.h"

namespace {

constexpr int FC_MAX_C = 4096;       // classes of the criterion
constexpr int FC_GROUPS = 16;        // frames of one workgroup pass: 16 lanes each, 256 threads
constexpr int FC_MAX_BLOCKS = 256;   // partial sums of the loss
constexpr int FC_GRAD_BLOCKS = 1024;
constexpr int FA_MAX_N = 16384;      // frames the rank statistic sorts in LDS
constexpr int FA_THREADS = 1024;

__device__ __forceinline__ float fc_row16_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 16));
    return v;
}

// logsumexp of one row by its 16 lanes (every lane of the DPP row is active): max, then sum exp(x - max), in float32
__device__ __forceinline__ float fc_logsumexp(const float* __restrict__ xr, int C, int sub) {
    float m = -INFINITY;
    for (int c = sub; c < C; c += 16) m = fmaxf(m, xr[c]);
    m = fc_row16_max(m);
    float s = 0.f;
    for (int c = sub; c < C; c += 16) s += expf(xr[c] - m);
    s = as_row16_sum(s);
    return m + logf(s);
}

// (the load stays behind a __restrict__ parameter of its own: without that scope the three kernels allocate registers differently)
__device__ __forceinline__ long fc_length(const int64_t* __restrict__ lengths, int b, int T) {
    return as_clamp_length<long>(lengths[b], T);
}

// ws: [0] the ticket (uint64), then per workgroup (numerator, denominator) as doubles
__global__ __launch_bounds__(256) void fc_loss_kernel(const float* __restrict__ x, long sx_t, long sx_b, int T, int B, int C,
                                                      const int64_t* __restrict__ targets, long ts, const int64_t* __restrict__ lengths,
                                                      const float* __restrict__ weight, long ignore, float eps, float* __restrict__ lse,
                                                      double* __restrict__ sums, unsigned long long* ws) {
    __shared__ double sh_num[FC_GROUPS], sh_den[FC_GROUPS];
    const int grp = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const long rows = (long)B * T;
    double num = 0.0, den = 0.0;
    for (long r = (long)blockIdx.x * FC_GROUPS + grp; r < rows; r += (long)gridDim.x * FC_GROUPS) {   // uniform per lane group
        const int b = (int)(r / T), t = (int)(r % T);
        if (t >= fc_length(lengths, b, T)) continue;
        const long y = targets[b * ts + t];
        if (y == ignore) continue;
        const float* xr = x + t * sx_t + b * sx_b;
        const float l = fc_logsumexp(xr, C, sub);
        const bool ok = y >= 0 && y < C;   // anything else never indexes x or weight: NaN
        const float wy = ok ? (weight ? weight[y] : 1.f) : NAN;
        float loss = wy * (l - (ok ? xr[y] : 0.f));
        if (eps != 0.f) {
            float a = 0.f;
            for (int c = sub; c < C; c += 16) a += (weight ? weight[c] : 1.f) * (l - xr[c]);
            a = as_row16_sum(a);
            loss = (1.f - eps) * loss + (eps / (float)C) * a;
        }
        if (sub == 0) {
            lse[r] = l;
            num += (double)loss;
            den += ok ? (double)wy : 0.0;
        }
    }
    if (sub == 0) {
        sh_num[grp] = num;
        sh_den[grp] = den;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    num = den = 0.0;
    for (int g = 0; g < FC_GROUPS; ++g) {
        num += sh_num[g];
        den += sh_den[g];
    }
    unsigned long long* part = ws + 1;
    __hip_atomic_store(part + 2 * blockIdx.x, (unsigned long long)__double_as_longlong(num), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part + 2 * blockIdx.x + 1, (unsigned long long)__double_as_longlong(den), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    // this thread alone stored the pair (write-through agent-scope stores): drained before the ticket says so
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long ticket = __hip_atomic_fetch_add(ws, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != gridDim.x - 1) return;
    __threadfence();   // the last workgroup: every pair is read by an agent-scope load below; added in workgroup order
    num = den = 0.0;
    for (unsigned g = 0; g < gridDim.x; ++g) {
        num += __longlong_as_double((long long)__hip_atomic_load(part + 2 * g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        den += __longlong_as_double((long long)__hip_atomic_load(part + 2 * g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    sums[0] = num;
    sums[1] = den;
    __hip_atomic_store(ws, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next call finds the ticket at zero
}

__global__ __launch_bounds__(256) void fc_grad_kernel(const float* __restrict__ x, long sx_t, long sx_b, int T, int B, int C,
                                                      const int64_t* __restrict__ targets, long ts, const int64_t* __restrict__ lengths,
                                                      const float* __restrict__ weight, long ignore, float eps,
                                                      const float* __restrict__ lse, const double* __restrict__ sums,
                                                      const float* __restrict__ gout, int mean, float* __restrict__ grad, long sg_t,
                                                      long sg_b) {
    const int grp = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const long rows = (long)B * T;
    const float scale = mean ? (float)((double)gout[0] / sums[1]) : gout[0];
    float wsum = (float)C;   // sum_k w[k] of the smoothing term
    if (eps != 0.f && weight) {
        float a = 0.f;
        for (int c = sub; c < C; c += 16) a += weight[c];
        wsum = as_row16_sum(a);
    }
    const float a2 = scale * (eps / (float)C);
    for (long r = (long)blockIdx.x * FC_GROUPS + grp; r < rows; r += (long)gridDim.x * FC_GROUPS) {
        const int b = (int)(r / T), t = (int)(r % T);
        float* gr = grad + t * sg_t + b * sg_b;
        const bool in = t < fc_length(lengths, b, T);
        const long y = in ? targets[b * ts + t] : ignore;
        if (!in || y == ignore) {
            for (int c = sub; c < C; c += 16) gr[c] = 0.f;
            continue;
        }
        const float* xr = x + t * sx_t + b * sx_b;
        const bool ok = y >= 0 && y < C;
        const float wy = ok ? (weight ? weight[y] : 1.f) : NAN;
        const float a1 = scale * (1.f - eps) * wy, l = lse[r];
        for (int c = sub; c < C; c += 16) {
            const float p = expf(xr[c] - l);
            float g = a1 * (p - (c == y ? 1.f : 0.f));
            if (eps != 0.f) g += a2 * (p * wsum - (weight ? weight[c] : 1.f));
            gr[c] = g;
        }
    }
}

// One workgroup per class.  fa_buf holds pow2ceil(cap) 64-bit entries: (key << 32) | positive flag, later
// (key << 32) | (negatives in front << 1) | positive flag.
__global__ __launch_bounds__(FA_THREADS) void fa_kernel(const float* __restrict__ x, long sx_t, long sx_b, int T, int B, int C,
                                                        const int64_t* __restrict__ targets, long ts, const int64_t* __restrict__ lengths,
                                                        long ignore, int cap, int64_t* __restrict__ n_pos, int64_t* __restrict__ n_neg,
                                                        int64_t* __restrict__ u2) {
    extern __shared__ unsigned long long fa_buf[];
    __shared__ unsigned fa_cnt, fa_wave[FA_THREADS / 64];
    __shared__ unsigned long long fa_red[FA_THREADS];
    const int cls = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) fa_cnt = 0;
    __syncthreads();
    const long rows = (long)B * T;
    for (long q = tid; q < rows; q += FA_THREADS) {
        const int b = (int)(q / T), t = (int)(q % T);
        if (t >= fc_length(lengths, b, T)) continue;
        const long y = targets[b * ts + t];
        if (y == ignore || y < 0 || y >= C) continue;
        const unsigned slot = atomicAdd(&fa_cnt, 1u);
        if (slot >= (unsigned)cap) continue;   // too many frames: refused below, nothing stored past the buffer
        const unsigned u = __float_as_uint(x[t * sx_t + b * sx_b + cls] + 0.f);   // -0 + 0 = +0: equal scores, equal keys
        const unsigned key = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
        fa_buf[slot] = ((unsigned long long)key << 32) | (y == cls ? 1u : 0u);
    }
    __syncthreads();
    const unsigned N = fa_cnt;   // block-uniform
    if (N > (unsigned)cap) {
        if (tid == 0) n_pos[cls] = n_neg[cls] = u2[cls] = -1;
        return;
    }
    unsigned npad = 2;
    while (npad < N) npad <<= 1;   // <= pow2ceil(cap): inside the buffer
    for (unsigned k = N + tid; k < npad; k += FA_THREADS) fa_buf[k] = ~0ull;   // above every real entry
    __syncthreads();
    for (unsigned k = 2; k <= npad; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned i = tid; i < npad / 2; i += FA_THREADS) {
                const unsigned lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const unsigned long long a = fa_buf[lo], c = fa_buf[hi];
                if ((a > c) == ((lo & k) == 0)) {
                    fa_buf[lo] = c;
                    fa_buf[hi] = a;
                }
            }
            __syncthreads();
        }
    // exclusive count of negatives in front of every entry: a contiguous chunk per thread, scanned across the workgroup
    const unsigned per = (npad + FA_THREADS - 1) / FA_THREADS;
    const unsigned k0 = min(tid * per, N), k1 = min(k0 + per, N);
    unsigned negs = 0;
    for (unsigned k = k0; k < k1; ++k) negs += 1u - (unsigned)(fa_buf[k] & 1u);
    const unsigned incl = as_wave_scan(negs, lane, AsAdd{});
    if (lane == 63) fa_wave[wave] = incl;
    __syncthreads();
    unsigned before = incl - negs, total = 0;
    for (int w = 0; w < FA_THREADS / 64; ++w) {
        if (w < wave) before += fa_wave[w];
        total += fa_wave[w];
    }
    for (unsigned k = k0; k < k1; ++k) {
        const unsigned long long e = fa_buf[k];
        fa_buf[k] = (e & 0xFFFFFFFF00000000ull) | ((unsigned long long)before << 1) | (e & 1u);
        before += 1u - (unsigned)(e & 1u);
    }
    __syncthreads();
    // a positive at k: all negatives of its tie group stand in front of it, so (negatives in front of k) = negatives <= its
    // score; (negatives in front of the group's first entry) = negatives below it
    unsigned long long acc = 0;
    for (unsigned k = k0; k < k1; ++k) {
        const unsigned long long e = fa_buf[k];
        if (!(e & 1u)) continue;
        const unsigned key = (unsigned)(e >> 32);
        unsigned lo = 0, hi = k;   // first entry with this key lies in [0, k]
        while (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            if ((unsigned)(fa_buf[mid] >> 32) < key) lo = mid + 1;
            else hi = mid;
        }
        acc += (unsigned)(fa_buf[lo] & 0xFFFFFFFFu) >> 1;
        acc += (unsigned)(e & 0xFFFFFFFFu) >> 1;
    }
    fa_red[tid] = acc;
    __syncthreads();
    for (int s = FA_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) fa_red[tid] += fa_red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        n_neg[cls] = total;
        n_pos[cls] = (int64_t)N - total;
        u2[cls] = (int64_t)fa_red[0];
    }
}

int fc_blocks(int32_t T, int32_t B, int cap) {
    const long b = ((long)T * B + FC_GROUPS - 1) / FC_GROUPS;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

int fc_check(const char* who, const float* x, int32_t T, int32_t B, int32_t C, const int64_t* targets, int64_t tgt_stride,
             const int64_t* lengths) {
    AS_REQUIRE(x && targets && lengths && T > 0 && B > 0 && C > 0 && tgt_stride >= T, AS_ERR_BAD_ARG, "%s: bad argument", who);
    return 0;
}

}  // namespace

extern "C" int64_t as_frame_ce_workspace_bytes(int32_t T, int32_t B) {
    if (T <= 0 || B <= 0) return 0;
    return 8 + 16L * fc_blocks(T, B, FC_MAX_BLOCKS);
}

extern "C" int as_frame_ce_loss(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, const int64_t* targets,
                                int64_t tgt_stride, const int64_t* lengths, const float* weight, int64_t ignore_index,
                                float label_smoothing, float* lse, double* sums, void* ws, int64_t ws_bytes, void* stream) {
    AS_TRY(fc_check("as_frame_ce_loss", x, T, B, C, targets, tgt_stride, lengths));
    AS_REQUIRE(lse && sums && label_smoothing >= 0.f && label_smoothing <= 1.f, AS_ERR_BAD_ARG, "as_frame_ce_loss: bad argument");
    AS_REQUIRE(C <= FC_MAX_C, AS_ERR_UNSUPPORTED, "as_frame_ce_loss: %d classes (at most %d supported)", C, FC_MAX_C);
    const int64_t need = as_frame_ce_workspace_bytes(T, B);
    AS_REQUIRE(ws && ws_bytes >= need && as_aligned16(ws), AS_ERR_WORKSPACE, "as_frame_ce_loss: workspace of %lld bytes, %lld needed",
               (long long)(ws ? ws_bytes : 0), (long long)need);
    hipLaunchKernelGGL(fc_loss_kernel, dim3(fc_blocks(T, B, FC_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, (long)sx_t, (long)sx_b,
                       T, B, C, targets, (long)tgt_stride, lengths, weight, (long)ignore_index, label_smoothing, lse, sums,
                       (unsigned long long*)ws);
    AS_LAUNCH_CHECK("as_frame_ce_loss");
    return 0;
}

extern "C" int as_frame_ce_grad(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, const int64_t* targets,
                                int64_t tgt_stride, const int64_t* lengths, const float* weight, int64_t ignore_index,
                                float label_smoothing, const float* lse, const double* sums, const float* gout, int32_t mean,
                                float* grad, int64_t sg_t, int64_t sg_b, void* stream) {
    AS_TRY(fc_check("as_frame_ce_grad", x, T, B, C, targets, tgt_stride, lengths));
    AS_REQUIRE(lse && sums && gout && grad && label_smoothing >= 0.f && label_smoothing <= 1.f, AS_ERR_BAD_ARG,
               "as_frame_ce_grad: bad argument");
    AS_REQUIRE(C <= FC_MAX_C, AS_ERR_UNSUPPORTED, "as_frame_ce_grad: %d classes (at most %d supported)", C, FC_MAX_C);
    hipLaunchKernelGGL(fc_grad_kernel, dim3(fc_blocks(T, B, FC_GRAD_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, (long)sx_t,
                       (long)sx_b, T, B, C, targets, (long)tgt_stride, lengths, weight, (long)ignore_index, label_smoothing, lse, sums,
                       gout, mean, grad, (long)sg_t, (long)sg_b);
    AS_LAUNCH_CHECK("as_frame_ce_grad");
    return 0;
}

extern "C" int as_frame_auroc(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, const int64_t* targets,
                              int64_t tgt_stride, const int64_t* lengths, int64_t ignore_index, int32_t max_frames, int64_t* n_pos,
                              int64_t* n_neg, int64_t* u2, void* stream) {
    AS_TRY(fc_check("as_frame_auroc", x, T, B, C, targets, tgt_stride, lengths));
    AS_REQUIRE(n_pos && n_neg && u2 && max_frames > 0, AS_ERR_BAD_ARG, "as_frame_auroc: bad argument");
    AS_REQUIRE(max_frames <= FA_MAX_N, AS_ERR_UNSUPPORTED, "as_frame_auroc: %d frames (at most %d supported)", max_frames, FA_MAX_N);
    int npad = 2;
    while (npad < max_frames) npad <<= 1;
    const int lds = npad * 8;
    if (lds > 65536 - 16384) {   // beside the 8.1 KiB of static LDS
        const hipError_t e = as_allow_dynamic_lds(fa_kernel, lds);
        AS_REQUIRE(e == hipSuccess, (int)e, "as_frame_auroc: %d bytes of LDS refused: %s", lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(fa_kernel, dim3(C), dim3(FA_THREADS), (size_t)lds, (hipStream_t)stream, x, (long)sx_t, (long)sx_b, T, B, C,
                       targets, (long)tgt_stride, lengths, (long)ignore_index, max_frames, n_pos, n_neg, u2);
    AS_LAUNCH_CHECK("as_frame_auroc");
    return 0;
}
