// CTC forced alignment: the Viterbi path of a known label sequence through the emissions, and what the articulation models read
// from it (one phoneme token per frame).  The reference has no alignment of its own: its per-frame sequences come from hand-made
// TextGrids (generate_vocal_tract_shape_v2.py:135-158).  One launch, one workgroup per utterance, in both input modes:
//
//   prologue   lse[t] = logsumexp_c x[t][b][c] of the utterance's own Tb rows, a thread per row, into LDS (logits mode; zeros
//              otherwise), so the recursion reads log-probabilities x - lse as ctc.hip's does.
//   recursion  ctc.hip's state graph (S = 2L + 1 states; stay, step, skip) in max-plus: thread k holds the SPT consecutive states
//              k*SPT .. k*SPT+SPT-1 in registers and needs the previous thread's last two -- __shfl_up inside one wave
//              (2 * max_target_length + 1 <= 256), the double-buffered LDS exchange with one barrier per step beyond that.  The
//              log-probabilities of CA_AHEAD steps are fetched one group ahead of the group being computed: they do not depend
//              on the state, so their latency stays off the time-sequential chain.  Each step leaves 2 bits per state (0 stay,
//              1 step, 2 skip), four states to a byte, rows of `pitch` bytes: in LDS when the utterance's table fits CA_LDS_BUDGET
//              next to the per-frame scratch, else in the caller's workspace.
//   trace-back thread 0 walks the table from the better end state to frame 0 and leaves the state of every frame in LDS.
//   expansion  a thread per frame: frame_index / frame_token / frame_filled are functions of that frame's state alone (on a
//              monotone path the entry before blank state s is s/2 - 1, and it has been emitted); the thread of a label state's
//              first frame walks that state's run for its span and the mean log-probability, summed in time order.  Every output
//              element has one writer: no atomics, repeats are bit-identical.
//
// Tie rules (part of the contract, tests/forced_align_fp64.py implements the same): candidates in the order stay, step, skip, a
// later one replaces the best so far only if strictly greater; at the end the label state S-2 wins when it is >= state S-1.
// Where torchaudio.functional.forced_align's rule is well defined these choices coincide with it; parity with it is unpinned.
#include <math.h>

#include "as_common.h"
#include "ctc_common.h"

namespace {

constexpr int CA_MAX_T = 8192;          // frames of one utterance: 6 bytes of LDS scratch per frame (lse, the path's state)
constexpr int CA_LDS_BUDGET = 57344;    // dynamic LDS of one workgroup (56 KiB of the 64 KiB a launch gets unasked; the rest is static)

inline int ca_pitch(int maxL) { return (int)as_round_up((2 * maxL + 1 + 3) / 4, 4); }   // bytes of one step's back-pointers
inline long ca_frame_bytes(int T) { return as_round_up(6L * T, 16); }                    // float lse[T], uint16 path[T]
inline bool ca_table_in_lds(int T, int maxL) { return ca_frame_bytes(T) + (long)T * ca_pitch(maxL) <= CA_LDS_BUDGET; }

template <int NT, int SPT, bool WS>
__global__ __launch_bounds__(NT) void ctc_align_kernel(const float* __restrict__ x, long sxt, long sxb, int T, int C, int logits,
                                                       const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                       const int64_t* __restrict__ in_len, const int64_t* __restrict__ tgt_len, int maxL,
                                                       int blank, unsigned char* __restrict__ ws, int pitch, float* __restrict__ score,
                                                       int* __restrict__ frame_index, int* __restrict__ frame_token,
                                                       int* __restrict__ frame_filled, int* __restrict__ spans,
                                                       float* __restrict__ span_score) {
    constexpr int AHEAD = SPT <= 4 ? 4 : 2;   // steps whose log-probabilities are in flight (AHEAD * SPT registers, twice)
    extern __shared__ __align__(16) unsigned char ca_lds[];
    __shared__ float xch[2][NT][2];
    __shared__ float fin[2];
    __shared__ int feasible;
    const int b = blockIdx.x, tid = threadIdx.x;
    float* lse = reinterpret_cast<float*>(ca_lds);                          // [T]: each row's normaliser
    unsigned short* path = reinterpret_cast<unsigned short*>(ca_lds + 4L * T);   // [T], the state of every frame
    unsigned char* lds_tab = ca_lds + (6L * T + 15) / 16 * 16;
    unsigned char* glb_tab = ws + (long)b * T * pitch;

    // rows of an utterance without an alignment: frames -1, spans (-1, -1), span scores NaN
    auto fill = [&](int t_from, int j_from) {
        for (int t = t_from + tid; t < T; t += NT) {
            if (frame_index) frame_index[(long)b * T + t] = -1;
            if (frame_token) frame_token[(long)b * T + t] = -1;
            if (frame_filled) frame_filled[(long)b * T + t] = -1;
        }
        for (int j = j_from + tid; j < maxL; j += NT) {
            if (spans) spans[((long)b * maxL + j) * 2] = -1, spans[((long)b * maxL + j) * 2 + 1] = -1;
            if (span_score) span_score[(long)b * maxL + j] = NAN;
        }
    };

    int L = 0, Tb = 0;
    long toff = 0;
    if (!ctc_sizes(in_len, tgt_len, targets, tgt_stride, b, T, maxL, L, Tb, toff)) {   // block-uniform
        if (tid == 0) score[b] = NAN;
        fill(0, 0);
        return;
    }
    if (Tb == 0) {
        if (tid == 0) score[b] = L == 0 ? 0.f : -INFINITY;
        fill(0, 0);
        return;
    }
    const float* xb = x + (long)b * sxb;
    if (logits) {
        // loads in groups of 8 with clamped addresses, so that a group's latencies overlap (a guarded load waits for itself)
        for (int t = tid; t < Tb; t += NT) {
            const float* xr = xb + t * sxt;
            float m = -INFINITY;
            for (int k0 = 0; k0 < C; k0 += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = xr[min(k0 + u, C - 1)];   // a repeated class does not change a maximum
#pragma unroll
                for (int u = 0; u < 8; ++u) m = fmaxf(m, v[u]);
            }
            float s = 0.f;
            if (m != -INFINITY)
                for (int k0 = 0; k0 < C; k0 += 8) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = xr[min(k0 + u, C - 1)];
#pragma unroll
                    for (int u = 0; u < 8; ++u) s += k0 + u < C ? expf(v[u] - m) : 0.f;
                }
            lse[t] = m == -INFINITY ? -INFINITY : m + logf(s);
        }
    } else {
        for (int t = tid; t < Tb; t += NT) lse[t] = 0.f;   // log-probabilities are used as given: x - 0 is x
    }
    __syncthreads();
    // a forbidden class (-inf) stays -inf whatever the row's normaliser is
    auto logp = [&](int t, int k) {
        const float v = xb[t * sxt + k];
        return v == -INFINITY ? v : v - lse[t];
    };

    // States past S - 1 are not masked: nothing moves down the state axis, the end and the trace-back start below S, so what they
    // hold never reaches a state that counts; they read the blank's column.  A label outside the classes is never read either:
    // its state takes -inf through `pen`, and with it every path.
    const int S = 2 * L + 1;
    int lab[SPT];
    bool skip[SPT];
    float pen[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int s = tid * SPT + i;
        const bool label = s < S && (s & 1);
        lab[i] = label ? (int)targets[toff + (s >> 1)] : blank;
        skip[i] = label && s >= 2 && lab[i] != (int)targets[toff + ((s - 2) >> 1)];
        pen[i] = 0.f;
        if (lab[i] < 0 || lab[i] >= C) lab[i] = blank, pen[i] = -INFINITY;
    }
    // Every load is issued whatever the state or the step (clamped step, in-range column) and its value is used arithmetically: a
    // guarded load becomes a branch that waits for its own data, which puts each latency back on the time-sequential chain.
    auto fetch = [&](float (&lp)[AHEAD][SPT], int t0) {
#pragma unroll
        for (int g = 0; g < AHEAD; ++g) {
            const int t = min(t0 + g, Tb - 1);
            const float* xr = xb + t * sxt;
            const float sub = lse[t];
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const float v = xr[lab[i]];
                lp[g][i] = (v == -INFINITY ? v : v - sub) + pen[i];
            }
        }
    };

    float a[SPT];
    float cur[AHEAD][SPT], nxt[AHEAD][SPT];
    fetch(cur, 0);
    for (int t0 = 0; t0 < Tb; t0 += AHEAD) {
        fetch(nxt, t0 + AHEAD);
#pragma unroll
        for (int g = 0; g < AHEAD; ++g) {
            const int t = t0 + g;
            if (t >= Tb) break;   // block-uniform
            if (t == 0) {
#pragma unroll
                for (int i = 0; i < SPT; ++i) a[i] = tid * SPT + i < 2 ? cur[g][i] : -INFINITY;
                continue;
            }
            float p1, p2;   // the previous thread's last state and the one before it
            if constexpr (NT == 64) {
                p1 = __shfl_up(a[SPT - 1], 1, 64);
                p2 = __shfl_up(a[SPT - 2], 1, 64);
                if (tid == 0) p1 = p2 = -INFINITY;
            } else {
                const int par = t & 1;
                xch[par][tid][0] = a[SPT - 1];
                xch[par][tid][1] = a[SPT - 2];
                __syncthreads();
                p1 = tid ? xch[par][tid - 1][0] : -INFINITY;
                p2 = tid ? xch[par][tid - 1][1] : -INFINITY;
            }
            float na[SPT];
            unsigned code = 0;
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const float m1 = i >= 1 ? a[i - 1] : p1;
                const float m2 = i >= 2 ? a[i - 2] : (i == 1 ? p1 : p2);
                float best = a[i];
                unsigned bp = 0;
                if (m1 > best) best = m1, bp = 1;
                if (skip[i] && m2 > best) best = m2, bp = 2;
                na[i] = best + cur[g][i];
                code |= bp << (2 * i);
            }
#pragma unroll
            for (int i = 0; i < SPT; ++i) a[i] = na[i];
            // thread k's SPT / 4 bytes of the row; bytes past the pitch belong to no state
            unsigned char* row = (WS ? glb_tab : lds_tab) + (long)t * pitch;
            if constexpr (SPT == 4) {
                if (tid < pitch) row[tid] = (unsigned char)code;
            } else {
                static_assert(SPT == 16, "a thread's back-pointers are one byte or one 32-bit word");
                if (4 * tid < pitch) reinterpret_cast<unsigned*>(row)[tid] = code;
            }
        }
#pragma unroll
        for (int g = 0; g < AHEAD; ++g)
#pragma unroll
            for (int i = 0; i < SPT; ++i) cur[g][i] = nxt[g][i];
    }

#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int s = tid * SPT + i;
        if (s == S - 1) fin[0] = a[i];
        if (s == S - 2) fin[1] = a[i];
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        int s = S - 1;
        float best = fin[0];
        if (S >= 2 && fin[1] >= best) s = S - 2, best = fin[1];
        const bool ok = best > -INFINITY;   // false for NaN too
        score[b] = best;
        feasible = ok;
        if (ok) {
            const unsigned char* tab = WS ? glb_tab : lds_tab;
            for (int t = Tb - 1; t > 0; --t) {
                path[t] = (unsigned short)s;
                s -= (tab[(long)t * pitch + (s >> 2)] >> (2 * (s & 3))) & 3;
            }
            path[0] = (unsigned short)s;
        }
    }
    __syncthreads();
    if (!feasible) {   // block-uniform
        fill(0, 0);
        return;
    }
    for (int t = tid; t < Tb; t += NT) {
        const int s = path[t], j = s >> 1;
        const bool label = s & 1;
        const int tok = label ? (int)targets[toff + j] : blank;
        if (frame_index) frame_index[(long)b * T + t] = label ? j : -1;
        if (frame_token) frame_token[(long)b * T + t] = tok;
        if (frame_filled) frame_filled[(long)b * T + t] = label ? j : (L == 0 ? -1 : (s == 0 ? 0 : j - 1));
        if (label && (spans || span_score) && (t == 0 || path[t - 1] != s)) {   // the first frame of entry j
            float sum = 0.f;
            int e = t;
            for (; e < Tb && path[e] == s; ++e) sum += logp(e, tok);
            if (spans) spans[((long)b * maxL + j) * 2] = t, spans[((long)b * maxL + j) * 2 + 1] = e;
            if (span_score) span_score[(long)b * maxL + j] = sum / (float)(e - t);
        }
    }
    fill(Tb, L);
}

}  // namespace

extern "C" int64_t as_ctc_align_workspace_bytes(int32_t T, int32_t B, int32_t max_target_length) {
    if (T <= 0 || B <= 0 || max_target_length < 0 || max_target_length > CTC_MAX_L || T > CA_MAX_T) return 0;
    if (ca_table_in_lds(T, max_target_length)) return 0;
    return (int64_t)B * T * ca_pitch(max_target_length);
}

extern "C" int as_ctc_align(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, int32_t logits,
                            const int64_t* targets, int64_t tgt_stride, const int64_t* input_lengths, const int64_t* target_lengths,
                            int32_t max_target_length, int32_t blank, void* ws, int64_t ws_bytes, float* score, int32_t* frame_index,
                            int32_t* frame_token, int32_t* frame_filled, int32_t* spans, float* span_score, void* stream) {
    const int maxL = max_target_length;
    AS_TRY(ctc_check("as_ctc_align", x, T, B, C, targets, input_lengths, target_lengths, maxL, blank, score && tgt_stride >= 0));
    AS_REQUIRE(T <= CA_MAX_T, AS_ERR_UNSUPPORTED, "as_ctc_align: %d frames (at most %d supported)", T, CA_MAX_T);
    const int64_t need = as_ctc_align_workspace_bytes(T, B, maxL);
    AS_REQUIRE(need == 0 || (ws && ws_bytes >= need), AS_ERR_WORKSPACE, "as_ctc_align: workspace of %lld bytes, %lld needed",
               (long long)(ws ? ws_bytes : 0), (long long)need);
    const int pitch = ca_pitch(maxL);
    const bool in_ws = need > 0;
    const size_t lds = (size_t)(ca_frame_bytes(T) + (in_ws ? 0 : (long)T * pitch));
    ctc_layout(maxL, [&](auto nt, auto spt) {
        constexpr int NT = decltype(nt)::value, SPT = decltype(spt)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(B), dim3(NT), lds, (hipStream_t)stream, x, (long)sx_t, (long)sx_b, T, C, logits, targets,
                               tgt_stride, input_lengths, target_lengths, maxL, blank, (unsigned char*)ws, pitch, score, frame_index,
                               frame_token, frame_filled, spans, span_score);
        };
        if (in_ws) launch(ctc_align_kernel<NT, SPT, true>);
        else launch(ctc_align_kernel<NT, SPT, false>);
    });
    AS_LAUNCH_CHECK("as_ctc_align");
    return 0;
}
