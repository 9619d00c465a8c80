// Phoneme-wise mean contour (reference phoneme_to_articulation/phoneme_wise_mean_contour/__init__.py): the baseline method of the
// thesis' result tables, fitted and evaluated on the device.
//
//   as_token_runs                 _calculate_tokens_lengths_and_positions (:19-29) for a whole flat data set or padded batch: a
//                                 segmented scan over the frames (forward max-scan of run heads, backward min-scan of run tails;
//                                 per-block aggregates, one wave scans the aggregates, the blocks finish), never a thread per
//                                 utterance
//   as_mean_contour_fit           the per-token mean of the sampled rows (forward_mean_contour's .mean(dim=0), :137), fused with
//                                 the compaction of the sample into the bank: every sampled frame is read once; fp64 sums in a
//                                 fixed order, fp32 table
//   as_mean_contour_fwd           table look-up per frame
//   as_mean_contour_weighted_fwd  forward_weighted_mean_contour (:86-122): out[q] = sum_k w_qk x_k / sum_k w_qk with
//                                 w_qk = exp(-|rel_k - rel_q|) over the bank rows of q's token -- attention with scalar keys and a
//                                 token-equality mask.  ONE launch: workgroup (token v, chunk of 256 consecutive frames, 256
//                                 columns) collects the chunk's queries of token v in LDS (order-preserving ballot compaction) and
//                                 streams the bank rows of v once per tile of 16 of them; the weights of 64 rows x 16 queries are
//                                 computed once per workgroup into LDS and broadcast, every thread owns one column and 16
//                                 accumulators.  Every exponent lies in [-1, 0]: no running maximum.
// Arithmetic: plain fp32 FMAs.  With 16 queries per bank row the loop does 32 flop per 4 bytes streamed (8 flop/B), below the fp32
// ridge of the part (~20 flop/B), and the tiles are ragged (1..16 queries): the matrix pipe has nothing to add.
#include "as_common.h"

#define MC_SCAN 1024   // frames per scan workgroup
#define MC_QC 256      // frames per query chunk = threads of the weighted kernel = columns per workgroup
#define MC_QT 16       // queries per tile (accumulators per thread)
#define MC_KC 64       // bank rows per weight chunk

namespace {

__device__ __forceinline__ int mc_scan_min_rev(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(v, o, 64);
        if (lane + o < 64) v = min(v, t);
    }
    return v;
}

// the utterance that holds frame i (first_row ascending): the last u with first_row[u] <= i; -1 if none or i is past its end
__device__ __forceinline__ int mc_utterance(const int64_t* first_row, const int32_t* lengths, int U, int64_t i) {
    int lo = 0, hi = U;   // first u with first_row[u] > i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (first_row[mid] <= i) lo = mid + 1; else hi = mid;
    }
    const int u = lo - 1;
    if (u < 0 || i >= first_row[u] + lengths[u]) return -1;
    return u;
}

// PASS 0: per-block aggregates (last head, first tail).  PASS 1: the scan with the carried-in values, and the outputs.
template <int PASS>
__global__ __launch_bounds__(MC_SCAN) void mc_runs_kernel(const int64_t* __restrict__ tokens, const int64_t* __restrict__ first_row,
                                                          const int32_t* __restrict__ lengths, int U, int64_t frames, int32_t* agg,
                                                          int32_t* __restrict__ abs_pos, int32_t* __restrict__ seq_len,
                                                          float* __restrict__ rel_pos) {
    __shared__ int s_head[MC_SCAN / 64], s_tail[MC_SCAN / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * MC_SCAN + tid;
    int head = -1, tail = INT32_MAX;
    bool valid = false;
    if (i < frames) {
        const int u = mc_utterance(first_row, lengths, U, i);
        valid = u >= 0;
        bool is_head = true, is_tail = true;
        if (valid) {
            const int64_t lo = first_row[u], hi = lo + lengths[u] - 1, tok = tokens[i];
            is_head = i == lo || tokens[i - 1] != tok;
            is_tail = i == hi || i + 1 >= frames || tokens[i + 1] != tok;
        }
        if (is_head) head = (int)i;
        if (is_tail) tail = (int)i;
    }
    head = as_wave_scan(head, lane, AsMax{});
    tail = mc_scan_min_rev(tail, lane);
    if (lane == 63) s_head[wave] = head;
    if (lane == 0) s_tail[wave] = tail;
    __syncthreads();
    if (PASS == 0) {
        if (tid == 0) {
            int h = -1, t = INT32_MAX;
            for (int w = 0; w < MC_SCAN / 64; ++w) { h = max(h, s_head[w]); t = min(t, s_tail[w]); }
            agg[2 * blockIdx.x] = h;
            agg[2 * blockIdx.x + 1] = t;
        }
        return;
    }
    const int nblocks = gridDim.x;
    int h = agg[2 * nblocks + 2 * blockIdx.x], t = agg[2 * nblocks + 2 * blockIdx.x + 1];   // carried in
    for (int w = 0; w < wave; ++w) h = max(h, s_head[w]);
    for (int w = wave + 1; w < MC_SCAN / 64; ++w) t = min(t, s_tail[w]);
    head = max(head, h);
    tail = min(tail, t);
    if (i < frames) {
        const int a = valid ? (int)i - head : 0, n = valid ? tail - head + 1 : 0;
        abs_pos[i] = a;
        seq_len[i] = n;
        rel_pos[i] = valid ? (float)a / (float)n : 0.f;
    }
}

// exclusive scans of the block aggregates by one wave: carry[b] = (max head of the blocks before b, min tail of the blocks after b)
__global__ __launch_bounds__(64) void mc_runs_carry_kernel(int32_t* agg, int nblocks) {
    const int lane = threadIdx.x;
    int32_t* carry = agg + 2 * nblocks;
    int run = -1;
    for (int b0 = 0; b0 < nblocks; b0 += 64) {
        const int b = b0 + lane;
        const int v = as_wave_scan(b < nblocks ? agg[2 * b] : -1, lane, AsMax{});
        int prev = __shfl_up(v, 1, 64);
        if (lane == 0) prev = -1;
        if (b < nblocks) carry[2 * b] = max(run, prev);
        run = max(run, __shfl(v, 63, 64));
    }
    run = INT32_MAX;
    for (int b0 = ((nblocks - 1) / 64) * 64; b0 >= 0; b0 -= 64) {
        const int b = b0 + lane;
        const int v = mc_scan_min_rev(b < nblocks ? agg[2 * b + 1] : INT32_MAX, lane);
        int next = __shfl_down(v, 1, 64);
        if (lane == 63) next = INT32_MAX;
        if (b < nblocks) carry[2 * b + 1] = min(run, next);
        run = min(run, __shfl(v, 0, 64));
    }
}

// workgroup (64 columns, token v): threadIdx.y = one of four row slices; fp64 partial sums combined in slice order
__global__ __launch_bounds__(256) void mc_fit_kernel(const float* __restrict__ src, const float* __restrict__ src_rel,
                                                     const int64_t* __restrict__ rows, const int64_t* __restrict__ off, int D,
                                                     float* bank_x, float* bank_rel, float* __restrict__ table) {
    __shared__ double s_part[4][64];
    const int v = blockIdx.y, x = threadIdx.x, y = threadIdx.y, d = blockIdx.x * 64 + x;
    const int64_t k0 = off[v], k1 = off[v + 1];
    double acc = 0.0;
    if (d < D) {
        for (int64_t k = k0 + y; k < k1; k += 4) {
            float val;
            if (rows) {
                val = src[rows[k] * D + d];
                bank_x[k * D + d] = val;
            } else {
                val = bank_x[k * D + d];
            }
            acc += (double)val;
        }
    }
    if (rows && blockIdx.x == 0 && x == 0)
        for (int64_t k = k0 + y; k < k1; k += 4) bank_rel[k] = src_rel[rows[k]];
    s_part[y][x] = acc;
    __syncthreads();
    if (y == 0 && d < D) {
        const double s = ((s_part[0][x] + s_part[1][x]) + s_part[2][x]) + s_part[3][x];
        table[(int64_t)v * D + d] = k1 > k0 ? (float)(s / (double)(k1 - k0)) : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void mc_fwd_kernel(const float* __restrict__ table, const int64_t* __restrict__ off,
                                                     const int64_t* __restrict__ tokens, const int32_t* __restrict__ lengths, int T,
                                                     int V, int D, float* __restrict__ out, int32_t* flag) {
    const int64_t q = blockIdx.x;
    const int b = (int)(q / T), t = (int)(q % T);
    const bool valid = t < lengths[b];
    const int64_t tok = valid ? tokens[q] : 0;
    const bool in_vocab = tok >= 0 && tok < V;
    float* o = out + q * D;
    if (valid && threadIdx.x == 0 && (!in_vocab || off[tok + 1] == off[tok])) atomicAdd(flag, 1);
    if (!valid || !in_vocab) {
        const float fill = valid ? __builtin_nanf("") : 0.f;
        for (int d = threadIdx.x; d < D; d += blockDim.x) o[d] = fill;
        return;
    }
    const float* row = table + tok * D;
    for (int d = threadIdx.x; d < D; d += blockDim.x) o[d] = row[d];
}

__global__ __launch_bounds__(MC_QC) void mc_weighted_kernel(const float* __restrict__ bank_x, const float* __restrict__ bank_rel,
                                                            const int64_t* __restrict__ off, const int64_t* __restrict__ tokens,
                                                            const float* __restrict__ rel, const int32_t* __restrict__ lengths,
                                                            int64_t Q, int T, int V, int D, float* __restrict__ out, int32_t* flag) {
    __shared__ int s_q[MC_QC];
    __shared__ float s_r[MC_QC];
    __shared__ unsigned char s_kind[MC_QC];
    __shared__ int s_count[MC_QC / 64];
    __shared__ __attribute__((aligned(16))) float s_w[MC_KC][MC_QT];
    __shared__ float s_sum[MC_QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v = blockIdx.x % V;
    const int64_t chunk = blockIdx.x / V, i = chunk * MC_QC + tid;
    const int d = blockIdx.y * MC_QC + tid;

    // ---- the chunk's queries of token v, in frame order
    bool match = false;
    int kind = 0;   // frames no token's workgroup writes: 1 padded (zeros), 2 token outside the vocabulary (NaN)
    float r = 0.f;
    if (i < Q) {
        const int b = (int)(i / T), t = (int)(i % T);
        if (t < lengths[b]) {
            const int64_t tok = tokens[i];
            match = tok == v;
            if (tok < 0 || tok >= V) kind = 2;
            r = rel[i];
        } else {
            kind = 1;
        }
    }
    const unsigned long long votes = __ballot(match);
    if (lane == 0) s_count[wave] = __popcll(votes);
    if (v == 0) s_kind[tid] = (unsigned char)kind;
    __syncthreads();
    int base = 0, n = 0;
    for (int w = 0; w < MC_QC / 64; ++w) {
        if (w < wave) base += s_count[w];
        n += s_count[w];
    }
    if (match) {
        const int pos = base + __popcll(votes & ((1ull << lane) - 1ull));
        s_q[pos] = tid;
        s_r[pos] = r;
    }
    if (v == 0) {   // one workgroup per (chunk, column tile) writes the frames that belong to no token
        int bad = 0;
        const int64_t left = Q - chunk * MC_QC;
        const int frames = (int)(left < MC_QC ? left : MC_QC);
        for (int j = 0; j < frames; ++j) {
            const int kj = s_kind[j];
            if (kj && d < D) out[(chunk * MC_QC + j) * D + d] = kj == 1 ? 0.f : __builtin_nanf("");
            bad += kj == 2;
        }
        if (bad && blockIdx.y == 0 && tid == 0) atomicAdd(flag, bad);
    }
    if (n == 0) return;
    __syncthreads();

    const int64_t k0 = off[v], k1 = off[v + 1];
    if (k0 == k1 && blockIdx.y == 0 && tid == 0) atomicAdd(flag, n);   // an empty bank: 0 / 0 below
    const int wq = tid >> 4, wj = tid & 15;   // this thread's share of the weights: query wq, rows wj, wj + 16, ...
    for (int q0 = 0; q0 < n; q0 += MC_QT) {
        const int nq = min(MC_QT, n - q0);
        const float rq = wq < nq ? s_r[q0 + wq] : 0.f;
        float acc[MC_QT];
#pragma unroll
        for (int j = 0; j < MC_QT; ++j) acc[j] = 0.f;
        float wpart = 0.f;
        for (int64_t kc = k0; kc < k1; kc += MC_KC) {
            __syncthreads();   // the previous chunk's weights are consumed
#pragma unroll
            for (int u = 0; u < MC_KC / 16; ++u) {
                const int kk = wj + 16 * u;
                const int64_t k = kc + kk;
                const float w = (k < k1 && wq < nq) ? expf(-fabsf(bank_rel[k] - rq)) : 0.f;
                s_w[kk][wq] = w;
                wpart += w;
            }
            __syncthreads();
            if (d < D) {
                const int rows = (int)(k1 - kc < MC_KC ? k1 - kc : MC_KC);
                const float* xp = bank_x + kc * D + d;
                for (int kk = 0; kk < rows; kk += 4) {
                    float x[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) x[u] = kk + u < rows ? xp[(int64_t)(kk + u) * D] : 0.f;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float4* wp = reinterpret_cast<const float4*>(s_w[kk + u]);
#pragma unroll
                        for (int j4 = 0; j4 < MC_QT / 4; ++j4) {
                            const float4 w = wp[j4];
                            acc[4 * j4 + 0] = fmaf(w.x, x[u], acc[4 * j4 + 0]);
                            acc[4 * j4 + 1] = fmaf(w.y, x[u], acc[4 * j4 + 1]);
                            acc[4 * j4 + 2] = fmaf(w.z, x[u], acc[4 * j4 + 2]);
                            acc[4 * j4 + 3] = fmaf(w.w, x[u], acc[4 * j4 + 3]);
                        }
                    }
                }
            }
        }
        // the denominators: the 16 lanes that share a query add their shares in a fixed order
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) wpart += __shfl_xor(wpart, o, 64);
        __syncthreads();
        if (wj == 0) s_sum[wq] = wpart;
        __syncthreads();
        if (d < D) {
#pragma unroll
            for (int j = 0; j < MC_QT; ++j)
                if (j < nq) out[(chunk * MC_QC + s_q[q0 + j]) * D + d] = acc[j] / s_sum[j];
        }
    }
}

}  // namespace

extern "C" int64_t as_token_runs_workspace_ints(int64_t frames) { return frames > 0 ? 4 * ((frames + MC_SCAN - 1) / MC_SCAN) : 0; }

extern "C" int as_token_runs(const int64_t* tokens, const int64_t* first_row, const int32_t* lengths, int32_t utterances, int64_t frames,
                             int32_t* abs_pos, int32_t* seq_len, float* rel_pos, int32_t* ws, void* stream) {
    AS_REQUIRE(utterances >= 0 && frames >= 0 && frames < INT32_MAX, AS_ERR_BAD_ARG, "as_token_runs: utterances=%d frames=%ld", utterances,
               (long)frames);
    if (frames == 0) return 0;
    AS_REQUIRE(tokens && abs_pos && seq_len && rel_pos && ws && (utterances == 0 || (first_row && lengths)), AS_ERR_BAD_ARG,
               "as_token_runs: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nblocks = as_cdiv(frames, MC_SCAN);
    AS_PROF("token_runs", st);
    hipLaunchKernelGGL(mc_runs_kernel<0>, dim3(nblocks), dim3(MC_SCAN), 0, st, tokens, first_row, lengths, utterances, frames, ws, abs_pos,
                       seq_len, rel_pos);
    AS_LAUNCH_CHECK("as_token_runs (aggregates)");
    hipLaunchKernelGGL(mc_runs_carry_kernel, dim3(1), dim3(64), 0, st, ws, nblocks);
    AS_LAUNCH_CHECK("as_token_runs (carries)");
    hipLaunchKernelGGL(mc_runs_kernel<1>, dim3(nblocks), dim3(MC_SCAN), 0, st, tokens, first_row, lengths, utterances, frames, ws, abs_pos,
                       seq_len, rel_pos);
    AS_LAUNCH_CHECK("as_token_runs (scan)");
    return 0;
}

extern "C" int as_mean_contour_fit(const float* src, const float* src_rel, const int64_t* rows, const int64_t* bank_offsets, int32_t vocab,
                                   int32_t D, float* bank_x, float* bank_rel, float* table, void* stream) {
    AS_REQUIRE(vocab >= 1 && vocab <= 65535 && D >= 1, AS_ERR_BAD_ARG, "as_mean_contour_fit: vocab=%d D=%d", vocab, D);
    AS_REQUIRE(bank_offsets && bank_x && table && (!rows || (src && src_rel && bank_rel)), AS_ERR_BAD_ARG,
               "as_mean_contour_fit: null pointer");
    hipStream_t st = (hipStream_t)stream;
    AS_PROF("mean_contour_fit", st);
    hipLaunchKernelGGL(mc_fit_kernel, dim3(as_cdiv(D, 64), vocab), dim3(64, 4), 0, st, src, src_rel, rows, bank_offsets, D, bank_x,
                       bank_rel, table);
    AS_LAUNCH_CHECK("as_mean_contour_fit");
    return 0;
}

extern "C" int as_mean_contour_fwd(const float* table, const int64_t* bank_offsets, const int64_t* tokens, const int32_t* lengths, int32_t B,
                                   int32_t T, int32_t vocab, int32_t D, float* out, int32_t* flag, void* stream) {
    AS_REQUIRE(B >= 0 && T >= 0 && vocab >= 1 && D >= 1 && (int64_t)B * T < INT32_MAX, AS_ERR_BAD_ARG,
               "as_mean_contour_fwd: B=%d T=%d vocab=%d D=%d", B, T, vocab, D);
    if ((int64_t)B * T == 0) return 0;
    AS_REQUIRE(table && bank_offsets && tokens && lengths && out && flag, AS_ERR_BAD_ARG, "as_mean_contour_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    AS_PROF("mean_contour_fwd", st);
    hipLaunchKernelGGL(mc_fwd_kernel, dim3((unsigned)(B * T)), dim3(256), 0, st, table, bank_offsets, tokens, lengths, T, vocab, D, out,
                       flag);
    AS_LAUNCH_CHECK("as_mean_contour_fwd");
    return 0;
}

extern "C" int as_mean_contour_weighted_fwd(const float* bank_x, const float* bank_rel, const int64_t* bank_offsets, const int64_t* tokens,
                                            const float* rel_pos, const int32_t* lengths, int32_t B, int32_t T, int32_t vocab, int32_t D,
                                            float* out, int32_t* flag, void* stream) {
    AS_REQUIRE(B >= 0 && T >= 0 && vocab >= 1 && D >= 1, AS_ERR_BAD_ARG, "as_mean_contour_weighted_fwd: B=%d T=%d vocab=%d D=%d", B, T,
               vocab, D);
    const int64_t Q = (int64_t)B * T;
    if (Q == 0) return 0;
    const int64_t chunks = (Q + MC_QC - 1) / MC_QC, tiles = (D + MC_QC - 1) / MC_QC;
    AS_REQUIRE(chunks * vocab < INT32_MAX && tiles <= 65535, AS_ERR_BAD_ARG,
               "as_mean_contour_weighted_fwd: %ld frames x %d tokens x %d columns exceed one launch", (long)Q, vocab, D);
    AS_REQUIRE(bank_x && bank_rel && bank_offsets && tokens && rel_pos && lengths && out && flag, AS_ERR_BAD_ARG,
               "as_mean_contour_weighted_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    AS_PROF("mean_contour_weighted_fwd", st);
    hipLaunchKernelGGL(mc_weighted_kernel, dim3((unsigned)(chunks * vocab), (unsigned)tiles), dim3(MC_QC), 0, st, bank_x, bank_rel,
                       bank_offsets, tokens, rel_pos, lengths, Q, T, vocab, D, out, flag);
    AS_LAUNCH_CHECK("as_mean_contour_weighted_fwd");
    return 0;
}
