// Evaluation of the phoneme recogniser on the device (reference phoneme_recognition/metrics.py, decoders.py and the matrices of
// phoneme_recognition/__init__.py): integer work only -- an arg-max, a compaction, a dynamic-programming table and histograms.
//
//   as_decode_top1       TopKDecoder.__call__ (decoders.py:36-42): re_argmax_kernel, one wave per frame with the lanes across the
//                        classes (torch's arg-max order: a NaN is the maximum, the lowest index wins among equals), then
//                        re_collapse_kernel, one workgroup per utterance: keep flags (first frame of a run, not blank) and an
//                        exclusive scan over the frames (wave scans + one LDS exchange), the raw arg-max row staged in LDS so the
//                        compaction may run in place.
//   as_edit_distance     torchmetrics' _edit_distance as word_error_rate calls it (metrics.py:135): one wave per pair, lane l owns
//                        the target columns l, l + 64, ... of the current table row in registers.  Row i follows from row i - 1 by
//                          x[j] = min(D[i-1][j] + 1, D[i-1][j-1] + (p_i != t_j)),   D[i][j] = min_{k <= j} (x[k] + j - k)
//                        -- the horizontal dependency is a prefix minimum of x[k] - k, six lane shifts per 64 columns -- so no
//                        table reaches memory and a row costs O(columns / 64) wave steps.
//   as_align_counts      substitution_matrix (metrics.py:324-392) after compute_transitions (:295-321): one wave per pair fills
//                        the same table row by row as uint16 (LDS where it fits the workgroup's 64 KB, else the caller's
//                        workspace), then walks back from the corner to the predecessor with the smallest entry (ties: diagonal,
//                        previous prediction row, previous target column -- the path the reference's shortest_path finds) and adds
//                        every move to the shared count matrix with integer atomic adds: order-free, bit-identical repeats.
//   as_confusion_counts  sklearn's confusion_matrix counts of compute_confusion_matrix (__init__.py:410-432): a per-workgroup LDS
//                        histogram flushed with integer atomic adds.
#include <limits.h>

#include "as_common.h"

namespace {

constexpr int RE_MAX_T = 8192;        // frames of one utterance: the raw arg-max row (int32) lives in LDS
constexpr int RE_MAX_P = 4096;        // predicted tokens per utterance
constexpr int RE_MAX_L = 2047;        // target tokens per utterance (the CTC kernel's limit): 2048 columns = 32 per lane
constexpr int RE_LDS_BYTES = 65536;   // dynamic LDS of one alignment workgroup
constexpr int RE_BIG = INT_MAX / 2;

// torch's arg-max order: does (a, ia) beat (b, ib)?
__device__ __forceinline__ bool re_better(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

__global__ __launch_bounds__(256) void re_argmax_kernel(const float* __restrict__ x, long sb, long st, int B, int T, int C,
                                                        const int64_t* __restrict__ lengths, int* __restrict__ raw) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // row = b * T + t
    const int lane = threadIdx.x & 63;
    if (row >= (long)B * T) return;   // wave-uniform
    const int b = (int)(row / T), t = (int)(row % T);
    const long len = as_clamp_length<long>(lengths ? lengths[b] : T, T);
    if (t >= len) {
        if (lane == 0) raw[row] = -1;
        return;
    }
    const float* xr = x + b * sb + t * st;
    float v = -INFINITY;
    int idx = INT_MAX;   // (-inf, INT_MAX) loses to every real (value, index)
    for (int k = lane; k < C; k += 64) {
        const float u = xr[k];
        if (re_better(u, k, v, idx)) { v = u; idx = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        const int ui = __shfl_xor(idx, o, 64);
        if (re_better(u, ui, v, idx)) { v = u; idx = ui; }
    }
    if (lane == 0) raw[row] = idx;
}

// raw [B][T] (-1 past the utterance's length) -> tokens [B][T]: runs collapsed, then blank dropped, padded with -1.  raw may be
// tokens itself: the row is staged in LDS before anything is written.
__global__ __launch_bounds__(256) void re_collapse_kernel(const int* raw, int T, int blank, int* tokens, int* __restrict__ counts) {
    extern __shared__ int re_row[];   // [T]
    __shared__ int wave_sum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* src = raw + (long)b * T;
    int* dst = tokens + (long)b * T;
    for (int t = tid; t < T; t += 256) re_row[t] = src[t];
    __syncthreads();
    const int chunk = (T + 255) / 256, t0 = tid * chunk, t1 = min(T, t0 + chunk);
    int n = 0;
    for (int t = t0; t < t1; ++t) {
        const int r = re_row[t];
        n += r >= 0 && r != blank && (t == 0 || r != re_row[t - 1]);
    }
    const int incl = as_wave_scan(n, lane, AsAdd{});
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = incl - n, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wave_sum[w];
        total += wave_sum[w];
    }
    for (int t = t0; t < t1; ++t) {
        const int r = re_row[t];
        if (r >= 0 && r != blank && (t == 0 || r != re_row[t - 1])) dst[before++] = r;
    }
    for (int t = total + tid; t < T; t += 256) dst[t] = -1;
    if (tid == 0) counts[b] = total;
}

__device__ __forceinline__ int re_class(const int* __restrict__ class_map, int n_map, int tok) {
    if (!class_map) return tok;
    return (tok >= 0 && tok < n_map) ? class_map[tok] : -1;
}
__device__ __forceinline__ int re_count(const int* __restrict__ counts, int i, int hi) {
    const int n = counts[i];
    return n < 0 ? 0 : (n > hi ? hi : n);
}

// KC: 64-column chunks per lane; column j = c * 64 + lane holds D[i][j] for j <= L
template <int KC>
__global__ __launch_bounds__(256) void re_edit_distance_kernel(const int* __restrict__ pred, int P_max, const int* __restrict__ pcount,
                                                               const int* __restrict__ tgt, int L_max, const int* __restrict__ tcount,
                                                               int B, const int* __restrict__ class_map, int n_map,
                                                               int* __restrict__ dist) {
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pair >= B) return;   // wave-uniform
    const int P = re_count(pcount, pair, P_max), L = re_count(tcount, pair, L_max);
    const int* pr = pred + (long)pair * P_max;
    const int* tr = tgt + (long)pair * L_max;
    int tg[KC], row[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        const int j = c * 64 + lane;
        tg[c] = (j >= 1 && j <= L) ? re_class(class_map, n_map, tr[j - 1]) : INT_MIN;   // INT_MIN: equal to no class
        row[c] = j;
    }
    for (int i0 = 0; i0 < P; i0 += 64) {
        // the next 64 prediction classes, one per lane, broadcast row by row
        const int mine = i0 + lane < P ? re_class(class_map, n_map, pr[i0 + lane]) : 0;
        const int rows = min(64, P - i0);
        for (int r = 0; r < rows; ++r) {
            const int p = __shfl(mine, r, 64), i = i0 + r + 1;
            int carry_old = 0, carry_min = RE_BIG;
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                if (c * 64 > L) break;   // wave-uniform
                const int j = c * 64 + lane, old = row[c];
                int up = __shfl_up(old, 1, 64);
                if (lane == 0) up = carry_old;
                carry_old = __shfl(old, 63, 64);
                int x = min(old + 1, up + (p != tg[c]));
                if (j == 0) x = i;
                int y = min(as_wave_scan(x - j, lane, AsMin{}), carry_min);
                carry_min = __shfl(y, 63, 64);
                row[c] = y + j;
            }
        }
    }
    int v = 0;
#pragma unroll
    for (int c = 0; c < KC; ++c)
        if (c == (L >> 6)) v = row[c];
    v = __shfl(v, L & 63, 64);
    if (lane == 0) dist[pair] = v;
}

// One wave per pair.  LDS: pc[P_max] and tc[L_max] (the class sequences), then the uint16 table if it fits (ws == NULL).
__global__ __launch_bounds__(64) void re_align_kernel(const int* __restrict__ pred, int P_max, const int* __restrict__ pcount,
                                                      const int* __restrict__ tgt, int L_max, const int* __restrict__ tcount,
                                                      const int* __restrict__ class_map, int n_map, int n_classes, uint16_t* ws,
                                                      int* counts, int* __restrict__ dist) {
    extern __shared__ int re_lds[];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int P = re_count(pcount, pair, P_max), L = re_count(tcount, pair, L_max), W = L + 1;
    int* pc = re_lds;
    int* tc = re_lds + P_max;
    uint16_t* tab = ws ? ws + (long)pair * (P_max + 1) * (L_max + 1) : reinterpret_cast<uint16_t*>(re_lds + P_max + L_max);
    for (int i = lane; i < P; i += 64) pc[i] = re_class(class_map, n_map, pred[(long)pair * P_max + i]);
    for (int j = lane; j < L; j += 64) tc[j] = re_class(class_map, n_map, tgt[(long)pair * L_max + j]);
    for (int j = lane; j <= L; j += 64) tab[j] = (uint16_t)j;
    __syncthreads();
    for (int i = 1; i <= P; ++i) {
        const int p = pc[i - 1];
        const uint16_t* prev = tab + (long)(i - 1) * W;
        uint16_t* cur = tab + (long)i * W;
        int carry_min = RE_BIG;
        for (int c0 = 0; c0 <= L; c0 += 64) {
            const int j = c0 + lane;
            int x = RE_BIG;   // columns past L: they follow every valid one in the scan and are not stored
            if (j == 0) x = i;
            else if (j <= L) x = min((int)prev[j] + 1, (int)prev[j - 1] + (p != tc[j - 1]));
            const int y = min(as_wave_scan(x - j, lane, AsMin{}), carry_min);
            carry_min = __shfl(y, 63, 64);
            if (j <= L) cur[j] = (uint16_t)(y + j);
        }
        __syncthreads();   // one wave: orders this row's stores before the next row's loads of other lanes' columns
    }
    if (lane != 0) return;
    dist[pair] = tab[(long)P * W + L];
    const int n1 = n_classes + 1;
    int i = P, j = L;
    while (i > 0 || j > 0) {
        const int d = (i > 0 && j > 0) ? tab[(long)(i - 1) * W + j - 1] : RE_BIG;
        const int u = i > 0 ? tab[(long)(i - 1) * W + j] : RE_BIG;
        const int l = j > 0 ? tab[(long)i * W + j - 1] : RE_BIG;
        if (d <= u && d <= l) {   // substitution or match: [target class][predicted class]
            const int t = tc[j - 1], p = pc[i - 1];
            if (t >= 0 && t < n_classes && p >= 0 && p < n_classes) atomicAdd(counts + t * n1 + p, 1);
            --i;
            --j;
        } else if (u <= l) {      // the target column stays: an inserted prediction, last row
            const int p = pc[i - 1];
            if (p >= 0 && p < n_classes) atomicAdd(counts + n_classes * n1 + p, 1);
            --i;
        } else {                  // the prediction row stays: a deleted target, last column
            const int t = tc[j - 1];
            if (t >= 0 && t < n_classes) atomicAdd(counts + t * n1 + n_classes, 1);
            --j;
        }
    }
}

constexpr int RE_HIST_LDS = 8192;   // counters of the per-workgroup histogram (n <= 90)

__global__ __launch_bounds__(256) void re_confusion_kernel(const int* __restrict__ argmax, int T, const int* __restrict__ targets, int S,
                                                           const int64_t* __restrict__ lengths, int B, const int* __restrict__ class_map,
                                                           int n_map, int n, int* counts) {
    __shared__ int hist[RE_HIST_LDS];
    const bool local = n * n <= RE_HIST_LDS;   // block-uniform
    if (local) {
        for (int k = threadIdx.x; k < n * n; k += 256) hist[k] = 0;
        __syncthreads();
    }
    const int F = min(T, S);
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < (long)B * F; q += (long)gridDim.x * 256) {
        const int b = (int)(q / F), t = (int)(q % F);
        if (lengths && t >= lengths[b]) continue;
        const int p = re_class(class_map, n_map, argmax[(long)b * T + t]);
        const int g = re_class(class_map, n_map, targets[(long)b * S + t]);
        if (p < 0 || p >= n || g < 0 || g >= n) continue;
        if (local) atomicAdd(hist + g * n + p, 1);
        else atomicAdd(counts + g * n + p, 1);
    }
    if (local) {
        __syncthreads();
        for (int k = threadIdx.x; k < n * n; k += 256)
            if (hist[k]) atomicAdd(counts + k, hist[k]);
    }
}

int re_pairs_check(const char* who, const int32_t* pred, int32_t P_max, const int32_t* pcount, const int32_t* tgt, int32_t L_max,
                   const int32_t* tcount, int32_t B, const int32_t* class_map, int32_t n_map) {
    AS_REQUIRE(pcount && tcount && B > 0 && P_max >= 0 && L_max >= 0 && (pred || P_max == 0) && (tgt || L_max == 0), AS_ERR_BAD_ARG,
               "%s: bad argument", who);
    AS_REQUIRE(!class_map || n_map > 0, AS_ERR_BAD_ARG, "%s: class_map without entries", who);
    AS_REQUIRE(P_max <= RE_MAX_P && L_max <= RE_MAX_L, AS_ERR_UNSUPPORTED, "%s: %d predicted / %d target tokens (at most %d / %d supported)",
               who, P_max, L_max, RE_MAX_P, RE_MAX_L);
    return 0;
}

long re_align_lds_bytes(int P_max, int L_max, bool with_table) {
    long bytes = 4L * (P_max + L_max);
    if (with_table) bytes += 2L * (P_max + 1) * (L_max + 1);
    return as_round_up(bytes > 0 ? bytes : 4, 4);
}

}  // namespace

extern "C" int as_decode_top1(const float* emissions, int64_t s_b, int64_t s_t, int32_t B, int32_t T, int32_t C, const int64_t* lengths,
                              int32_t blank, int32_t* tokens, int32_t* counts, int32_t* argmax, void* stream) {
    AS_REQUIRE(emissions && tokens && counts && B > 0 && T > 0 && C > 0, AS_ERR_BAD_ARG, "as_decode_top1: bad argument");
    AS_REQUIRE(T <= RE_MAX_T, AS_ERR_UNSUPPORTED, "as_decode_top1: %d frames (at most %d supported)", T, RE_MAX_T);
    hipStream_t st = (hipStream_t)stream;
    int32_t* raw = argmax ? argmax : tokens;
    hipLaunchKernelGGL(re_argmax_kernel, dim3(as_cdiv((long)B * T, 4)), dim3(256), 0, st, emissions, (long)s_b, (long)s_t, B, T, C,
                       lengths, raw);
    AS_LAUNCH_CHECK("as_decode_top1");
    hipLaunchKernelGGL(re_collapse_kernel, dim3(B), dim3(256), (size_t)T * sizeof(int), st, raw, T, blank, tokens, counts);
    AS_LAUNCH_CHECK("as_decode_top1");
    return 0;
}

extern "C" int as_edit_distance(const int32_t* pred, int32_t P_max, const int32_t* pred_counts, const int32_t* target, int32_t L_max,
                                const int32_t* target_counts, int32_t B, const int32_t* class_map, int32_t n_map, int32_t* dist,
                                void* stream) {
    AS_TRY(re_pairs_check("as_edit_distance", pred, P_max, pred_counts, target, L_max, target_counts, B, class_map, n_map));
    AS_REQUIRE(dist, AS_ERR_BAD_ARG, "as_edit_distance: null output");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(as_cdiv(B, 4)), block(256);
    const int chunks = L_max / 64 + 1;   // columns 0 .. L_max
    as_up_to<1, 2, 4, 8, 16, 32>(chunks, [&](auto kc) {
        hipLaunchKernelGGL((re_edit_distance_kernel<decltype(kc)::value>), grid, block, 0, st, pred, P_max, pred_counts, target, L_max,
                           target_counts, B, class_map, n_map, dist);
    });
    AS_LAUNCH_CHECK("as_edit_distance");
    return 0;
}

extern "C" int64_t as_align_workspace_bytes(int32_t B, int32_t P_max, int32_t L_max) {
    if (B <= 0 || P_max < 0 || L_max < 0 || P_max > RE_MAX_P || L_max > RE_MAX_L) return 0;
    if (re_align_lds_bytes(P_max, L_max, true) <= RE_LDS_BYTES) return 0;
    return 2L * B * (P_max + 1) * (L_max + 1);
}

extern "C" int as_align_counts(const int32_t* pred, int32_t P_max, const int32_t* pred_counts, const int32_t* target, int32_t L_max,
                               const int32_t* target_counts, int32_t B, const int32_t* class_map, int32_t n_map, int32_t n_classes,
                               int32_t* counts, int32_t* dist, void* ws, int64_t ws_bytes, void* stream) {
    AS_TRY(re_pairs_check("as_align_counts", pred, P_max, pred_counts, target, L_max, target_counts, B, class_map, n_map));
    AS_REQUIRE(counts && dist && n_classes > 0, AS_ERR_BAD_ARG, "as_align_counts: bad argument");
    const int64_t need = as_align_workspace_bytes(B, P_max, L_max);
    AS_REQUIRE(need == 0 || (ws && ws_bytes >= need), AS_ERR_WORKSPACE, "as_align_counts: workspace of %lld bytes, %lld needed",
               (long long)(ws ? ws_bytes : 0), (long long)need);
    const long lds = re_align_lds_bytes(P_max, L_max, need == 0);
    hipLaunchKernelGGL(re_align_kernel, dim3(B), dim3(64), (size_t)lds, (hipStream_t)stream, pred, P_max, pred_counts, target, L_max,
                       target_counts, class_map, n_map, n_classes, need ? (uint16_t*)ws : nullptr, counts, dist);
    AS_LAUNCH_CHECK("as_align_counts");
    return 0;
}

extern "C" int as_confusion_counts(const int32_t* argmax, int32_t T, const int32_t* targets, int32_t S, const int64_t* lengths, int32_t B,
                                   const int32_t* class_map, int32_t n_map, int32_t n, int32_t* counts, void* stream) {
    AS_REQUIRE(argmax && targets && counts && B > 0 && T > 0 && S > 0 && n > 0, AS_ERR_BAD_ARG, "as_confusion_counts: bad argument");
    AS_REQUIRE(!class_map || n_map > 0, AS_ERR_BAD_ARG, "as_confusion_counts: class_map without entries");
    AS_REQUIRE(n <= 32768, AS_ERR_UNSUPPORTED, "as_confusion_counts: %d classes (at most 32768 supported)", n);
    const long frames = (long)B * (T < S ? T : S);
    const int blocks = (int)(frames / 2048 + 1 > 256 ? 256 : frames / 2048 + 1);
    hipLaunchKernelGGL(re_confusion_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, argmax, T, targets, S, lengths, B, class_map,
                       n_map, n, counts);
    AS_LAUNCH_CHECK("as_confusion_counts");
    return 0;
}
