// CTC beam search over prefixes (flashlight's lexicon-free decoder with a zero language model, which the reference reaches through
// torchaudio.models.decoder.ctc_decoder(lexicon=None), test_phoneme_recognition.py:84-91): the N most probable labellings of every
// utterance with their scores.  tests/ctc_beam_fp64.py is the contract in float64.  One launch, one workgroup of 256 threads per
// utterance, every per-frame state in LDS:
//
//   rows       the emission rows of CB_G frames are loaded one group ahead of the group being searched (they do not depend on the
//              beam), and each wave then prepares one row: log / log-softmax (input modes 1 / 2), the rank of every class (higher
//              value first, equal values in ascending class index), the K shortlisted classes with their scores (+ sil_score) and
//              the row's best shortlisted score.  Global-memory latency stays off the frame-sequential chain.
//   live set   at most beam_size prefixes, each a node of the utterance's trie with the scores of its two hypotheses (ends in a
//              label / ends in blank), kept RELATIVE to the frame's best; the running offset is a double.
//   slots      a dense table, K + 2 slots per live prefix: 0 "stay on blank" -> (p, blank), 1 "repeat" -> (p, label), 2 + r
//              "extend by shortlisted class r" -> (p + n, label).  One thread gathers a slot's contributions in a fixed order
//              (own label hypothesis, own blank hypothesis; the repeat slot then takes its live parent's extension by the same
//              label, whose own slot stays empty), drops those below best - beam_threshold and merges the rest by max or
//              logaddexp.  No float atomics: repeats are bit-identical.
//   prune      the beam_size-th largest slot by a radix select over order-preserving integer keys, 8 bits a pass over the bits
//              that the frame's scores occupy (integer LDS counters: counts do not depend on arrival order), equal keys in slot
//              order; survivors are compacted in slot order by a block scan.
//   trie       node = (parent << 7 | label) in the workspace, with an open-addressed table (parent, label) -> node beside it, so
//              that a prefix that died and comes back finds its old node: identity is the label sequence.  Only surviving new
//              prefixes look up or insert (at most beam_size per frame, one thread each, integer compare-and-swap).
//   result     both hypotheses of a prefix are merged, the prefixes ranked by score (equal scores in live order), the first nbest
//              written by walking parents.  Every output element has one writer.
#include <math.h>

#include "as_common.h"

namespace {

constexpr int CB_NT = 256;
constexpr int CB_MAX_BEAM = 64;
constexpr int CB_MAX_C = 128;
constexpr int CB_MAX_T = 8192;
constexpr int CB_G = CB_NT / 64;                          // rows prepared per group: one per wave
constexpr int CB_SLOTS = CB_MAX_BEAM * (CB_MAX_C + 2);    // 33 KB of float slots at the largest beam and shortlist

inline int64_t cb_nodes(int T, int beam) { return (int64_t)beam * T + 1; }   // the root and at most beam new prefixes a frame
inline int cb_table_log2(int T, int beam) {
    int l = 6;
    while (((int64_t)1 << l) < 2 * cb_nodes(T, beam)) ++l;
    return l;
}

// order-preserving integer key of a slot's score; an empty slot (-inf, or NaN) is 0 and below every valid key
__device__ __forceinline__ unsigned cb_key(float v) {
    if (!(v > -INFINITY)) return 0u;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float cb_merge(float acc, float v, bool log_add) {
    if (!log_add) return fmaxf(acc, v);
    if (acc == -INFINITY) return v;
    const float m = fmaxf(acc, v);
    return m + log1pf(expf(fminf(acc, v) - m));
}

// exclusive scan of one int per thread over the workgroup, and the total; two barriers, the first of which also orders what the
// caller wrote to LDS before the call
__device__ __forceinline__ int cb_scan(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = as_wave_scan(v, lane, AsAdd{});
    __syncthreads();
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < CB_G; ++k) {
        const int s = wsum[k];
        if (k < w) base += s;
        total += s;
    }
    return base + inc - v;
}

__global__ __launch_bounds__(CB_NT) void ctc_beam_kernel(const float* __restrict__ x, long sxt, long sxb, int T, int C, int mode,
                                                         const int64_t* __restrict__ lengths, int blank, int sil, float sil_score,
                                                         int beam, int K, float thr, int log_add, int nbest,
                                                         int* __restrict__ tokens, int* __restrict__ counts,
                                                         float* __restrict__ scores, int* __restrict__ num_hyps,
                                                         int* __restrict__ ws, long ws_ints, long n_nodes, int table_log2) {
    __shared__ float val[CB_SLOTS];
    __shared__ int hist[256];
    __shared__ float raw[CB_G][CB_MAX_C];
    __shared__ float sl_x[2][CB_G][CB_MAX_C];          // score of the shortlisted class of rank r (sil_score added)
    __shared__ short sl_class[2][CB_G][CB_MAX_C];      // class of rank r
    __shared__ short rank_of[2][CB_G][CB_MAX_C];       // rank of a class, -1 outside the shortlist
    __shared__ float row_best[2][CB_G];
    __shared__ int eNode[2][CB_MAX_BEAM], eLast[2][CB_MAX_BEAM], ePar[2][CB_MAX_BEAM];   // node, last label, parent's node
    __shared__ float eF[2][CB_MAX_BEAM], eT[2][CB_MAX_BEAM];                             // ends in a label / ends in blank
    __shared__ int ePending[CB_MAX_BEAM];
    __shared__ int parIdx[CB_MAX_BEAM];
    __shared__ unsigned childMask[CB_MAX_BEAM][CB_MAX_C / 32];
    __shared__ int wsum[CB_G];
    __shared__ float redMax[CB_G], redMin[CB_G];
    __shared__ int redCnt[CB_G];
    __shared__ int sel[2];
    __shared__ float fin[CB_MAX_BEAM];
    __shared__ int ord[CB_MAX_BEAM], lens[CB_MAX_BEAM];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* nodekey = ws + (long)b * ws_ints;        // [n_nodes]: parent << 7 | label
    int* table = nodekey + n_nodes;               // [1 << table_log2]: node, 0 = empty (the root is never looked up)
    const unsigned table_mask = (1u << table_log2) - 1u;
    const float* xb = x + (long)b * sxb;
    const int Tb = as_clamp_length(lengths ? (int)lengths[b] : T, T);

    for (long k = tid; k < ((long)1 << table_log2); k += CB_NT) table[k] = 0;
    for (int k = tid; k < 2 * CB_G * CB_MAX_C; k += CB_NT) (&sl_class[0][0][0])[k] = 0;
    if (tid == 0) {
        eNode[0][0] = 0, eLast[0][0] = -1, ePar[0][0] = -1, eF[0][0] = 0.f, eT[0][0] = -INFINITY, parIdx[0] = -1;
        for (int k = 0; k < CB_MAX_C / 32; ++k) childMask[0][k] = 0u;
    }
    __threadfence_block();
    __syncthreads();

    // every load is issued whatever the row (clamped frame, clamped class): wave w takes frame t0 + w, a lane two classes
    auto fetch = [&](int t0, float& v0, float& v1) {
        const int t = min(t0 + wave, Tb - 1);
        const float* xr = xb + (long)t * sxt;
        v0 = xr[min(lane, C - 1)];
        v1 = xr[min(lane + 64, C - 1)];
    };
    // the row of frame t0 + wave into buffer `buf`: block-uniform barriers, the work itself is one wave's
    auto prepare = [&](int t0, int buf, float v0, float v1) {
        const bool live = t0 + wave < Tb;
        const int c0 = lane, c1 = lane + 64;
        if (!(v0 == v0)) v0 = -INFINITY;     // NaN counts as a forbidden class
        if (!(v1 == v1)) v1 = -INFINITY;
        if (c0 >= C) v0 = -INFINITY;
        if (c1 >= C) v1 = -INFINITY;
        if (mode == 1) {
            v0 = v0 > 0.f ? logf(v0) : -INFINITY;
            v1 = v1 > 0.f ? logf(v1) : -INFINITY;
        } else if (mode == 2) {
            const float m = as_wave_max(fmaxf(v0, v1));
            float s = 0.f;
            if (m > -INFINITY) s = (c0 < C ? expf(v0 - m) : 0.f) + (c1 < C ? expf(v1 - m) : 0.f);
            s = as_wave_sum(s);
            const float lse = m > -INFINITY ? m + logf(s) : 0.f;
            if (v0 > -INFINITY) v0 -= lse;
            if (v1 > -INFINITY) v1 -= lse;
        }
        if (live) {
            if (c0 < C) raw[wave][c0] = v0;
            if (c1 < C) raw[wave][c1] = v1;
        }
        __syncthreads();
        float best = -INFINITY;
        if (live) {
            int r0 = 0, r1 = 0;
            for (int c = 0; c < C; ++c) {
                const float o = raw[wave][c];
                r0 += (o > v0) || (o == v0 && c < c0);
                r1 += (o > v1) || (o == v1 && c < c1);
            }
            if (c0 < C) {
                const float xs = v0 + (c0 == sil ? sil_score : 0.f);
                rank_of[buf][wave][c0] = (short)(r0 < K ? r0 : -1);
                if (r0 < K) sl_class[buf][wave][r0] = (short)c0, sl_x[buf][wave][r0] = xs, best = xs;
            }
            if (c1 < C) {
                const float xs = v1 + (c1 == sil ? sil_score : 0.f);
                rank_of[buf][wave][c1] = (short)(r1 < K ? r1 : -1);
                if (r1 < K) sl_class[buf][wave][r1] = (short)c1, sl_x[buf][wave][r1] = xs, best = fmaxf(best, xs);
            }
        }
        best = as_wave_max(best);
        if (live && lane == 0) row_best[buf][wave] = best;
        __syncthreads();
    };

    int P = 1, cur = 0, node_count = 1;
    double offset = 0.0;
    bool dead = false;
    const int W = K + 2;

    if (Tb > 0) {
        float v0, v1;
        fetch(0, v0, v1);
        prepare(0, 0, v0, v1);
    }
    for (int t0 = 0; t0 < Tb && !dead; t0 += CB_G) {
        const int buf = (t0 / CB_G) & 1;
        float n0, n1;
        fetch(t0 + CB_G, n0, n1);
        for (int g = 0; g < CB_G && t0 + g < Tb; ++g) {       // block-uniform
            const float* sx = sl_x[buf][g];
            const short* sc = sl_class[buf][g];
            const short* rk = rank_of[buf][g];
            const int nxt = cur ^ 1;
            const int ns = P * W;
            const float cut = row_best[buf][g] - thr;          // the best single contribution is the best live score, 0, + row_best

            // ---- slots
            float lmax = -INFINITY, lmin = INFINITY;
            int lcnt = 0;
            for (int s = tid; s < ns; s += CB_NT) {
                const int i = s / W, j = s - i * W;
                const float sF = eF[cur][i], sT = eT[cur][i];
                const int last = eLast[cur][i];
                float acc = -INFINITY;
                auto add = [&](float sc_, float xv) {
                    const float v = sc_ + xv;
                    if (v > -INFINITY && v >= cut) acc = cb_merge(acc, v, log_add);
                };
                if (j == 0) {
                    const int rb = rk[blank];
                    if (rb >= 0) add(sF, sx[rb]), add(sT, sx[rb]);
                } else if (j == 1) {
                    const int rl = last >= 0 ? rk[last] : -1;
                    if (rl >= 0) {
                        const float xv = sx[rl];
                        add(sF, xv);
                        const int pi = parIdx[i];
                        if (pi >= 0) {
                            if (eLast[cur][pi] != last) add(eF[cur][pi], xv);
                            add(eT[cur][pi], xv);
                        }
                    }
                } else {
                    const int n = sc[j - 2];
                    if (n != blank && !((childMask[i][n >> 5] >> (n & 31)) & 1u)) {
                        const float xv = sx[j - 2];
                        if (n != last) add(sF, xv);
                        add(sT, xv);
                    }
                }
                val[s] = acc;
                if (cb_key(acc)) ++lcnt, lmax = fmaxf(lmax, acc), lmin = fminf(lmin, acc);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lmax = fmaxf(lmax, __shfl_xor(lmax, o, 64));
                lmin = fminf(lmin, __shfl_xor(lmin, o, 64));
                lcnt += __shfl_xor(lcnt, o, 64);
            }
            if (lane == 0) redMax[wave] = lmax, redMin[wave] = lmin, redCnt[wave] = lcnt;
            __syncthreads();
            float vmax = -INFINITY, vmin = INFINITY;
            int nvalid = 0;
#pragma unroll
            for (int k = 0; k < CB_G; ++k) vmax = fmaxf(vmax, redMax[k]), vmin = fminf(vmin, redMin[k]), nvalid += redCnt[k];
            if (nvalid == 0) {        // every contribution of this frame is -inf: no hypothesis
                dead = true;
                break;
            }

            // ---- prune to the beam: kth = the key of rank beam, need = how many slots of that key survive (in slot order)
            const int per = (ns + CB_NT - 1) / CB_NT, c_lo = min(tid * per, ns), c_hi = min(c_lo + per, ns);
            if (nvalid > beam) {
                // Keys are taken relative to the frame's smallest, and the passes cover only the bits that the frame's scores
                // occupy, the first with a full 8-bit digit: the top byte of a float's key is nearly the same for every score of a
                // frame, which would put a pass's counts on two or three counters.
                const unsigned kmin = cb_key(vmin), range = cb_key(vmax) - kmin;
                unsigned prefix = 0u;                  // (kth - kmin) >> shift: the bits decided so far
                int kk = beam, shift = 32 - __clz(range);
                while (shift > 0) {                    // block-uniform
                    const int hi = shift;              // candidates: (key - kmin) >> hi == prefix
                    shift = max(shift - 8, 0);
                    const unsigned digits = (1u << (hi - shift)) - 1u;
                    hist[tid] = 0;
                    __syncthreads();
                    for (int s = tid; s < ns; s += CB_NT) {
                        const unsigned key = cb_key(val[s]);
                        if (!key) continue;
                        const unsigned rel = key - kmin;
                        if (hi >= 32 || (rel >> hi) == prefix) atomicAdd(&hist[(rel >> shift) & digits], 1);
                    }
                    __syncthreads();
                    if (wave == 0) {                   // descending digits, four to a lane
                        int h4[4], sum = 0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) h4[k] = hist[255 - (4 * lane + k)], sum += h4[k];
                        int inc = sum;
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const int n = __shfl_up(inc, o, 64);
                            if (lane >= o) inc += n;
                        }
                        int before = inc - sum;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (before < kk && kk <= before + h4[k]) sel[0] = 255 - (4 * lane + k), sel[1] = kk - before;
                            before += h4[k];
                        }
                    }
                    __syncthreads();
                    prefix = (prefix << (hi - shift)) | (unsigned)sel[0];
                    kk = sel[1];                       // (the next pass writes sel two barriers from here)
                }
                const unsigned kth = kmin + prefix;
                int eq = 0;
                for (int s = c_lo; s < c_hi; ++s) eq += cb_key(val[s]) == kth;
                int total;
                int eq_before = cb_scan(eq, wsum, total);
                for (int s = c_lo; s < c_hi; ++s) {
                    const unsigned key = cb_key(val[s]);
                    if (key < kth || (key == kth && eq_before++ >= kk)) val[s] = -INFINITY;
                }
                __syncthreads();
            }

            // ---- the new live set, in slot order: one entry per surviving prefix
            int heads = 0;
            for (int s = c_lo; s < c_hi; ++s) {
                if (!cb_key(val[s])) continue;
                const int j = s % W;
                if (j >= 2) heads += 0x10001;                           // low half: entries, high half: new prefixes
                else if (j == 0 || !cb_key(val[s - 1])) heads += 1;
            }
            int total;
            int at = cb_scan(heads, wsum, total);
            // exactly min(beam, nvalid) slots survive the prune, so there are at most beam <= CB_MAX_BEAM entries
            const int P_new = total & 0xFFFF, n_ext = total >> 16;
            for (int s = c_lo; s < c_hi; ++s) {
                if (!cb_key(val[s])) continue;
                const int i = s / W, j = s - i * W;
                const int e = at & 0xFFFF;
                if (j >= 2) {
                    eNode[nxt][e] = node_count + (at >> 16), eLast[nxt][e] = sc[j - 2], ePar[nxt][e] = eNode[cur][i];
                    eF[nxt][e] = val[s] - vmax, eT[nxt][e] = -INFINITY, ePending[e] = 1;
                    at += 0x10001;
                } else if (j == 0 || !cb_key(val[s - 1])) {
                    eNode[nxt][e] = eNode[cur][i], eLast[nxt][e] = eLast[cur][i], ePar[nxt][e] = ePar[cur][i], ePending[e] = 0;
                    if (j == 0) {
                        eT[nxt][e] = val[s] - vmax;
                        eF[nxt][e] = cb_key(val[s + 1]) ? val[s + 1] - vmax : -INFINITY;   // slot 1 of the same prefix: W >= 3
                    } else {
                        eF[nxt][e] = val[s] - vmax, eT[nxt][e] = -INFINITY;
                    }
                    at += 1;
                }
            }
            __syncthreads();

            // ---- a new prefix finds its node or takes the one reserved for it
            if (tid < P_new && ePending[tid]) {
                const int mine = eNode[nxt][tid];
                const int key = (ePar[nxt][tid] << 7) | eLast[nxt][tid];
                unsigned h = ((unsigned)key * 0x9E3779B1u) >> (32 - table_log2);
                int found = mine;
                bool done = false;
                for (unsigned probe = 0; probe <= table_mask && !done; ++probe, h = (h + 1u) & table_mask) {
                    int seen = table[h];
                    if (seen == 0) {
                        seen = atomicCAS(&table[h], 0, mine);
                        if (seen == 0) nodekey[mine] = key, done = true;   // read from the next frame on, behind this frame's barriers
                    }
                    // a node of this frame belongs to another new prefix: its key is not read
                    if (!done && seen < node_count && nodekey[seen] == key) found = seen, done = true;
                }
                eNode[nxt][tid] = found;
            }
            if (tid < CB_MAX_BEAM)
                for (int k = 0; k < CB_MAX_C / 32; ++k) childMask[tid][k] = 0u;
            __threadfence_block();
            __syncthreads();
            if (tid < P_new) {
                const int par = ePar[nxt][tid];
                int pi = -1;
                if (eNode[nxt][tid] != 0)
                    for (int k = 0; k < P_new; ++k)
                        if (eNode[nxt][k] == par) pi = k;
                parIdx[tid] = pi;
                if (pi >= 0) atomicOr(&childMask[pi][eLast[nxt][tid] >> 5], 1u << (eLast[nxt][tid] & 31));
            }
            node_count += n_ext;
            offset += (double)vmax;
            P = P_new;
            cur = nxt;
            __syncthreads();
        }
        if (dead) break;
        if (t0 + CB_G < Tb) prepare(t0 + CB_G, buf ^ 1, n0, n1);   // block-uniform
    }

    // ---- result
    int nh = 0;
    if (!dead) {
        if (tid < P) fin[tid] = cb_merge(cb_merge(-INFINITY, eF[cur][tid], log_add), eT[cur][tid], log_add);
        __syncthreads();
        int r = 0;
        if (tid < P) {
            const float mine = fin[tid];
            for (int k = 0; k < P; ++k) r += (fin[k] > mine) || (fin[k] == mine && k < tid);
            ord[tid] = -1;
        }
        __syncthreads();
        if (tid < P) ord[r] = tid;         // r < P, and the ranks are a permutation (equal scores go in live order)
        __syncthreads();
        nh = min(P, nbest);
    }
    if (tid < nh) {
        const int i = ord[tid];
        int len = 0;
        if (i >= 0) {
            for (int node = eNode[cur][i]; node != 0 && len < T; node = nodekey[node] >> 7) ++len;
            int at = len;
            for (int node = eNode[cur][i]; node != 0 && at > 0; node = nodekey[node] >> 7)
                tokens[((long)b * nbest + tid) * T + --at] = nodekey[node] & 127;
        }
        lens[tid] = len;
        counts[(long)b * nbest + tid] = len;
        scores[(long)b * nbest + tid] = i >= 0 ? (float)(offset + (double)fin[i]) : -INFINITY;
    }
    for (int r = nh + tid; r < nbest; r += CB_NT) counts[(long)b * nbest + r] = 0, scores[(long)b * nbest + r] = -INFINITY;
    if (tid == 0) num_hyps[b] = nh;
    __syncthreads();
    for (long k = tid; k < (long)nbest * T; k += CB_NT) {
        const long r = k / T, p = k - r * T;
        if (r >= nh || p >= lens[r]) tokens[(long)b * nbest * T + k] = -1;
    }
}

}  // namespace

extern "C" int64_t as_ctc_beam_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t beam_size) {
    if (T <= 0 || B <= 0 || C < 2 || C > CB_MAX_C || beam_size < 1 || beam_size > CB_MAX_BEAM || T > CB_MAX_T) return 0;
    return (int64_t)B * 4 * (cb_nodes(T, beam_size) + ((int64_t)1 << cb_table_log2(T, beam_size)));
}

extern "C" int as_ctc_beam_search(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, int32_t input_mode,
                                  const int64_t* lengths, int32_t blank, int32_t sil, float sil_score, int32_t beam_size,
                                  int32_t beam_size_token, float beam_threshold, int32_t log_add, int32_t nbest, int32_t* tokens,
                                  int32_t* counts, float* scores, int32_t* num_hyps, void* ws, int64_t ws_bytes, void* stream) {
    AS_REQUIRE(x && tokens && counts && scores && num_hyps && T > 0 && B > 0 && C > 0 && blank >= 0 && blank < C && nbest >= 1 &&
                   input_mode >= 0 && input_mode <= 2 && sil < C && beam_threshold >= 0.f && sil_score == sil_score,
               AS_ERR_BAD_ARG, "as_ctc_beam_search: bad argument");
    AS_REQUIRE(beam_size >= 1 && beam_size <= CB_MAX_BEAM, AS_ERR_UNSUPPORTED, "as_ctc_beam_search: beam_size %d (1 to %d supported)",
               beam_size, CB_MAX_BEAM);
    AS_REQUIRE(C >= 2 && C <= CB_MAX_C, AS_ERR_UNSUPPORTED, "as_ctc_beam_search: %d classes (2 to %d supported)", C, CB_MAX_C);
    AS_REQUIRE(beam_size_token >= 1 && beam_size_token <= C, AS_ERR_UNSUPPORTED,
               "as_ctc_beam_search: beam_size_token %d (1 to the %d classes supported)", beam_size_token, C);
    AS_REQUIRE(T <= CB_MAX_T, AS_ERR_UNSUPPORTED, "as_ctc_beam_search: %d frames (at most %d supported)", T, CB_MAX_T);
    const int64_t need = as_ctc_beam_workspace_bytes(T, B, C, beam_size);
    AS_REQUIRE(ws && ws_bytes >= need, AS_ERR_WORKSPACE, "as_ctc_beam_search: workspace of %lld bytes, %lld needed",
               (long long)(ws ? ws_bytes : 0), (long long)need);
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(CB_NT), 0, (hipStream_t)stream, x, (long)sx_t, (long)sx_b, T, C, input_mode,
                       lengths, blank, sil, sil_score, beam_size, beam_size_token, beam_threshold, log_add, nbest, tokens, counts,
                       scores, num_hyps, (int*)ws, (long)(need / 4 / B), (long)cb_nodes(T, beam_size), cb_table_log2(T, beam_size));
    AS_LAUNCH_CHECK("as_ctc_beam_search");
    return 0;
}
