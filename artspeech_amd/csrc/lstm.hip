// Bidirectional LSTM recurrence (nn.LSTM semantics: the RNNType.LSTM switch of phoneme_to_articulation/__init__.py:47-49,
// used by principal_components/models/rnn.py:58-68) as persistent kernels, same design as gru.hip: one workgroup per
// (utterance, direction) walks its own sequence (packed-sequence semantics for free), W_hh (4H x H) lives in registers
// spread over 4 lanes per hidden unit (128 weight VGPRs per lane at H = 128), h_{t-1} in double-buffered LDS with one
// barrier per step, dot products finished with DPP quad permutes, operands loaded two steps ahead (three name-rotated sets, gru.hip).
//   i = s(gi_i + W_hi h + b_hi)  f = s(gi_f + ...)  g = tanh(gi_g + ...)  o = s(gi_o + ...)     (gate row order i, f, g, o)
//   c' = f c + i g,  h' = o tanh(c')
// The forward keeps i, f, g, o and c' per frame for the backward; the backward emits the pre-activation gradients (one
// array: input- and hidden-side pre-activations share them), weight gradients are time-batched GEMMs over them.
#include <cstdlib>

#include "as_common.h"
#include "as_device.h"
#include "rnn_plain.h"

namespace {

constexpr int LPU = 4;  // lanes per hidden unit

template <int H, bool TRAIN, bool TOK>
__global__ __launch_bounds__(LPU * H) void lstm_fwd_kernel(const float* __restrict__ gi, const int64_t* __restrict__ tokens,
                                                           long tok_stride, const float* __restrict__ w_hh,
                                                           const float* __restrict__ b_hh, const int* __restrict__ lengths, int T,
                                                           float* __restrict__ y, float* __restrict__ gates) {
    constexpr int CW = 4 * LPU, NC = H / CW, NT = LPU * H;
    __shared__ __attribute__((aligned(16))) float hbuf[2][H];
    extern __shared__ int tok_s[];
    const int b = blockIdx.x, dir = blockIdx.y;
    const int tid = threadIdx.x, j = tid / LPU, q = tid % LPU;
    const int len = lengths[b];

    f32x2 w[4][NC * 2];
    {
        const float* wd = w_hh + (long)dir * 4 * H * H;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(wd + (long)(g * H + j) * H + CW * c + 4 * q);
                w[g][2 * c] = f32x2{v.x, v.y};
                w[g][2 * c + 1] = f32x2{v.z, v.w};
            }
    }
    float bh[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bh[g] = b_hh[dir * 4 * H + g * H + j] * (1.0f / LPU);   // a quarter per lane of the unit: see below

    for (long i = (long)len * H + tid; i < (long)T * H; i += NT)  // pad_packed_sequence: zeros at padded frames
        y[((long)b * T + i / H) * 2 * H + dir * H + (i % H)] = 0.f;
    if (tid < H) hbuf[0][tid] = 0.f;
    if (TOK)
        for (int t = tid; t < len; t += NT) tok_s[t] = (int)tokens[(long)b * tok_stride + t] * (8 * H);   // element offset of the row
    __syncthreads();
    if (len <= 0) return;

    const int t0 = dir ? len - 1 : 0;
    const int dt = dir ? -1 : 1;
    float* yb = y + dir * H + j;                    // + frame * 2H
    float* gb = gates + (long)dir * 5 * H + j;      // + frame * 10H, planes i, f, g, o, c' at + plane * H   (TRAIN)
    const float* gib = gi + (long)dir * 4 * H + j;  // + row * 8H
    const int m0 = q == 0 ? -1 : 0, m1 = q == 1 ? -1 : 0, m2 = q == 2 ? -1 : 0, m3 = q == 3 ? -1 : 0;

    float cst = 0.f;
    struct Gi { float x[4]; };
    // input projection of step u (clamped to the last step: the look-ahead stays inside the sequence)
    auto load_step = [&](int u) {
        const int uc = u < len ? u : len - 1;
        const int tu = t0 + uc * dt;
        const float* p = gib + (TOK ? (long)tok_s[tu] : ((long)b * T + tu) * 8 * H);
        Gi v;
#pragma unroll
        for (int g = 0; g < 4; ++g) v.x[g] = p[g * H];
        return v;
    };
    // One recurrent step: consumes `ci` (loaded two steps ago), starts the loads of step s + 2 into `fill` (gru.hip: the
    // operand sets rotate by NAME through a loop unrolled by three, so that nothing consumes a load in the step that issued it)
    auto step = [&](int s, const Gi& ci, Gi& fill) {
        const int cur = s & 1;
        const long fr = (long)b * T + t0 + (long)s * dt;
        fill = load_step(s + 2);
        const float4* hp = reinterpret_cast<const float4*>(hbuf[cur]);
        // the recurrent biases ride in as the accumulators' start value (gru.hip)
        f32x2 a[4] = {{bh[0], 0.f}, {bh[1], 0.f}, {bh[2], 0.f}, {bh[3], 0.f}};
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += 8) {  // 8 LDS reads in flight, then their FMAs
            float4 hv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (c0 + u < NC) hv[u] = hp[LPU * (c0 + u) + q];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (c0 + u < NC) {
                    const int c = c0 + u;
                    const f32x2 lo = {hv[u].x, hv[u].y}, hi = {hv[u].z, hv[u].w};
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        a[g] = __builtin_elementwise_fma(w[g][2 * c], lo, a[g]);
                        a[g] = __builtin_elementwise_fma(w[g][2 * c + 1], hi, a[g]);
                    }
                }
        }
        const float gi_ = as_sigmoid(ci.x[0] + as_quad_sum<4>(a[0].x + a[0].y));
        const float gf = as_sigmoid(ci.x[1] + as_quad_sum<4>(a[1].x + a[1].y));
        const float gg = as_tanh(ci.x[2] + as_quad_sum<4>(a[2].x + a[2].y));
        const float go = as_sigmoid(ci.x[3] + as_quad_sum<4>(a[3].x + a[3].y));
        cst = gf * cst + gi_ * gg;
        const float hnew = go * as_tanh(cst);
        hbuf[cur ^ 1][j] = hnew;  // the lanes of a unit hold identical values: all store the same word
        yb[fr * 2 * H] = hnew;
        if (TRAIN) {
            const int gv = (__float_as_int(gi_) & m0) | (__float_as_int(gf) & m1) | (__float_as_int(gg) & m2) | (__float_as_int(go) & m3);
            gb[fr * 10 * H + q * H] = __int_as_float(gv);
            gb[fr * 10 * H + 4 * H] = cst;
        }
        __syncthreads();
    };
    Gi a = load_step(0), bq = load_step(1), c;
    int s = 0;
    for (; s + 2 < len; s += 3) {
        step(s, a, c);
        step(s + 1, bq, a);
        step(s + 2, c, bq);
    }
    if (s < len) step(s, a, c);
    if (s + 1 < len) step(s + 1, bq, a);
}

// Backward recurrence, row layout (as gru_bwd_row_kernel): the earlier layout of 4 lanes per unit read all 4H gate gradients
// per lane quad (32 ds_read_b128 per lane and step at H = 128: 8 waves x 32 x 8 cycles = 2048 LDS cycles, the whole measured step).  Here a
// ROW of 16 lanes owns 4 hidden units: a lane holds W_hh^T for those 4 columns over 1/16 of the gate rows (the same 128
// weight VGPRs), reads 4H/16 gate gradients per step (8 ds_read_b128) and the four partial sums are reduce-scattered over
// the row (rotated accumulator slots: 5 DPP adds, every lane ends with the total of ITS unit).  Lane r of a row plays
// unit 4 row + (r & 3), gate plane r >> 2 (i, f, g, o).
template <int H>
__global__ __launch_bounds__(4 * H) void lstm_bwd_row_kernel(const float* __restrict__ dy, const float* __restrict__ gates,
                                                             const float* __restrict__ w_hh, const int* __restrict__ lengths, int T,
                                                             float* __restrict__ dg) {
    constexpr int NT = 4 * H;
    constexpr int VL = 4 * H / 16;  // gate rows per lane
    constexpr int NCH = VL / 4;     // ds_read_b128 per lane and step
    __shared__ __attribute__((aligned(16))) float gbuf[2][4 * H];
    const int b = blockIdx.x, dir = blockIdx.y;
    const int tid = threadIdx.x, row = tid >> 4, r = tid & 15;
    const int qp = r & 3, pl = r >> 2;
    const int k0 = row * 4, k = k0 + qp;
    const int len = lengths[b];

    // slot s works for unit (s + qp) & 3; wt[s][2c + pp] = W_hh^T rows (c*16 + r)*4 + 2pp (+1) of that unit's column
    f32x2 wt[4][VL / 2];
    {
        const float* wd = w_hh + (long)dir * 4 * H * H;
        auto pick = [](const float4& v, int u) { return u == 0 ? v.x : u == 1 ? v.y : u == 2 ? v.z : v.w; };
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                const int i = (c * 16 + r) * 4 + 2 * pp;
                const float4 lo = *reinterpret_cast<const float4*>(wd + (long)i * H + k0);
                const float4 hi = *reinterpret_cast<const float4*>(wd + (long)(i + 1) * H + k0);
#pragma unroll
                for (int sl = 0; sl < 4; ++sl) wt[sl][2 * c + pp] = f32x2{pick(lo, (sl + qp) & 3), pick(hi, (sl + qp) & 3)};
            }
    }
    for (long i = (long)len * 4 * H + tid; i < (long)T * 4 * H; i += NT) {  // padded frames feed the time-batched GEMMs as zeros
        const long t = i / (4 * H), c = i % (4 * H);
        dg[(((long)b * T + t) * 2 + dir) * 4 * H + c] = 0.f;
    }
    if (len <= 0) return;

    const int t0 = dir ? 0 : len - 1;  // opposite to the forward walk
    const int dt = dir ? 1 : -1;
    const float* gtb = gates + (long)dir * 5 * H + k;        // + frame * 10H
    const float* dyb = dy + dir * H + k;                     // + frame * 2H
    float* dgb = dg + (long)dir * 4 * H + pl * H + k;        // + frame * 8H
    const int m0 = pl == 0 ? -1 : 0, m1 = pl == 1 ? -1 : 0, m2 = pl == 2 ? -1 : 0, m3 = pl == 3 ? -1 : 0;
    // nothing in `load` may consume a loaded value (gru.hip): has_prev is applied where cprev is used
    struct In { float i, f, g, o, c, cprev, dyv; bool has_prev; };
    auto load = [&](long fr, bool has_prev) {
        In v;
        const float* gp = gtb + fr * 10 * H;
        v.i = gp[0]; v.f = gp[H]; v.g = gp[2 * H]; v.o = gp[3 * H]; v.c = gp[4 * H];
        v.cprev = gtb[(fr + (has_prev ? dt : 0)) * 10 * H + 4 * H];
        v.has_prev = has_prev;
        v.dyv = dyb[fr * 2 * H];
        return v;
    };
    const long fbase = (long)b * T + t0;   // frame of step u: fbase + u * dt
    float dh = 0.f, dc = 0.f;
    auto load_step = [&](int u) {
        const int uc = u < len ? u : len - 1;
        return load(fbase + (long)uc * dt, uc + 1 < len);
    };
    // One step: consumes `cur_in` (loaded two steps ago), starts the loads of step s + 2 into `fill`
    auto step = [&](int s, const In& cur_in, In& fill) {
        const int cur = s & 1;
        const long fr = fbase + (long)s * dt;
        fill = load_step(s + 2);
        const float dht = dh + cur_in.dyv;
        const float tc = as_tanh(cur_in.c);
        const float dct = dc + dht * cur_in.o * (1.f - tc * tc);
        const float p_o = dht * tc * cur_in.o * (1.f - cur_in.o);
        const float p_i = dct * cur_in.g * cur_in.i * (1.f - cur_in.i);
        const float p_f = dct * (cur_in.has_prev ? cur_in.cprev : 0.f) * cur_in.f * (1.f - cur_in.f);
        const float p_g = dct * cur_in.i * (1.f - cur_in.g * cur_in.g);
        dc = dct * cur_in.f;
        const float v = __int_as_float((__float_as_int(p_i) & m0) | (__float_as_int(p_f) & m1) | (__float_as_int(p_g) & m2) |
                                       (__float_as_int(p_o) & m3));
        gbuf[cur][pl * H + k] = v;
        dgb[fr * 8 * H] = v;
        __syncthreads();
        const float4* gq = reinterpret_cast<const float4*>(gbuf[cur]);
        float4 gv[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) gv[c] = gq[c * 16 + r];
        __builtin_amdgcn_sched_barrier(0);
        f32x2 a[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const f32x2 lo = {gv[c].x, gv[c].y}, hi = {gv[c].z, gv[c].w};
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) {
                a[sl] = __builtin_elementwise_fma(wt[sl][2 * c], lo, a[sl]);
                a[sl] = __builtin_elementwise_fma(wt[sl][2 * c + 1], hi, a[sl]);
            }
        }
        float acc = a[0].x + a[0].y;
        acc = as_dpp_add<0x39>(acc, a[3].x + a[3].y);   // quad_perm [1,2,3,0]
        acc = as_dpp_add<0x4E>(acc, a[2].x + a[2].y);   // quad_perm [2,3,0,1]
        acc = as_dpp_add<0x93>(acc, a[1].x + a[1].y);   // quad_perm [3,0,1,2]
        acc = as_dpp_add<0x124>(acc, acc);              // row_ror 4
        acc = as_dpp_add<0x128>(acc, acc);              // row_ror 8
        dh = acc;
        // gbuf is double buffered: the next step writes gbuf[cur^1], whose readers all passed the barrier above
    };
    In a = load_step(0), bq = load_step(1), c;
    int s = 0;
    for (; s + 2 < len; s += 3) {
        step(s, a, c);
        step(s + 1, bq, a);
        step(s + 2, c, bq);
    }
    if (s < len) step(s, a, c);
    if (s + 1 < len) step(s + 1, bq, a);
}

// ---- any hidden size (nn.LSTM takes any, principal_components/models/rnn.py:58-68): the plain kernels, rnn_plain.h.

// Forward: four adjacent lanes share a hidden unit; lane q takes the 16-byte chunks q, q + 4, ... of the unit's four W_hh rows
// (the quad reads 64 consecutive bytes of a row), four chunks = 16 global loads in flight per pass.  H % 4 == 0.  (The loop
// is gru.hip's for four gates, written out here too: see there.)
template <bool TRAIN, bool TOK>
__global__ __launch_bounds__(GEN_THREADS) void lstm_fwd_generic_kernel(const float* __restrict__ gi, const int64_t* __restrict__ tokens,
                                                                      long tok_stride, const float* __restrict__ w_hh,
                                                                      const float* __restrict__ b_hh, const int* __restrict__ lengths,
                                                                      int T, int H, float* __restrict__ y, float* __restrict__ gates) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];   // LSTM_FWD_LDS_PER_UNIT
    float* cb = gsm + 2 * H;
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int q = tid & 3;
    const int len = lengths[b];
    for (long i = (long)len * H + tid; i < (long)T * H; i += GEN_THREADS)   // pad_packed_sequence: exact zeros
        y[((long)b * T + i / H) * 2 * H + dir * H + (i % H)] = 0.f;
    for (int j = tid; j < 3 * H; j += GEN_THREADS) gsm[j] = 0.f;
    __syncthreads();
    if (len <= 0) return;
    const float* wd = w_hh + (long)dir * 4 * H * H;
    const float* bd = b_hh + (long)dir * 4 * H;
    const int nch = H >> 2;   // 16-byte chunks per row
    for (int s = 0; s < len; ++s) {
        const int t = dir ? len - 1 - s : s;
        const long frame = (long)b * T + t;
        const float* hc = gsm + (s & 1) * H;
        float* hn_ = gsm + ((s & 1) ^ 1) * H;
        const float* gr = gi + (TOK ? tokens[(long)b * tok_stride + t] * 8L * H : frame * 8L * H) + (long)dir * 4 * H;
        for (int j = tid >> 2; j < H; j += GEN_THREADS / 4) {   // (the four lanes of a quad share j: the DPP sums are whole)
            const float4* h4 = reinterpret_cast<const float4*>(hc);
            float sg[4] = {0.f, 0.f, 0.f, 0.f};
            for (int c0 = q; c0 < nch; c0 += 16) {
                float4 wv[4][4], hv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {      // branch-free: chunks beyond the row re-read its last one against a zero h
                    const int cc = c0 + 4 * u;
                    const int ci = cc < nch ? cc : nch - 1;
#pragma unroll
                    for (int g = 0; g < 4; ++g) wv[g][u] = reinterpret_cast<const float4*>(wd + (long)(g * H + j) * H)[ci];
                    hv[u] = h4[ci];
                    if (cc >= nch) hv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        sg[g] += wv[g][u].x * hv[u].x + wv[g][u].y * hv[u].y + wv[g][u].z * hv[u].z + wv[g][u].w * hv[u].w;
            }
            const float gi_ = as_sigmoid(gr[j] + as_quad_sum<4>(sg[0]) + bd[j]);
            const float gf = as_sigmoid(gr[H + j] + as_quad_sum<4>(sg[1]) + bd[H + j]);
            const float gg = as_tanh(gr[2 * H + j] + as_quad_sum<4>(sg[2]) + bd[2 * H + j]);
            const float go = as_sigmoid(gr[3 * H + j] + as_quad_sum<4>(sg[3]) + bd[3 * H + j]);
            const float cnew = gf * cb[j] + gi_ * gg;     // (the quad's lanes read c before lane 0 writes it: one wave, program order)
            const float hnew = go * as_tanh(cnew);
            if (q == 0) {
                cb[j] = cnew;
                hn_[j] = hnew;
                y[frame * 2 * H + dir * H + j] = hnew;
                if (TRAIN) {
                    float* gp = gates + frame * 10L * H + (long)dir * 5 * H + j;
                    gp[0] = gi_; gp[H] = gf; gp[2 * H] = gg; gp[3 * H] = go; gp[4 * H] = cnew;
                }
            }
        }
        __syncthreads();
    }
}

// Backward: the four gate gradients of a step by one thread per hidden unit; then dh = W_hh^T p (rnn_plain_matvec_bwd).
__global__ __launch_bounds__(GEN_THREADS) void lstm_bwd_generic_kernel(const float* __restrict__ dy, const float* __restrict__ gates,
                                                                      const float* __restrict__ w_hh, const int* __restrict__ lengths,
                                                                      int T, int H, float* __restrict__ dg) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];   // LSTM_BWD_LDS_PER_UNIT
    float* gb = gsm;
    float* dhb = gsm + 4 * H;
    float* dcb = gsm + 5 * H;
    float* part = gsm + 6 * H;
    const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const int len = lengths[b];
    rnn_plain_zero_padded(dg, nullptr, b, T, len, 4 * H, 8L * H, (long)dir * 4 * H, tid);
    for (int j = tid; j < 2 * H; j += GEN_THREADS) dhb[j] = 0.f;   // dh and dc
    __syncthreads();
    if (len <= 0) return;
    const float* wd = w_hh + (long)dir * 4 * H * H;
    const int dt = dir ? 1 : -1;   // opposite to the forward walk; c_prev of frame t is the cell state of the frame visited NEXT
    for (int s = 0; s < len; ++s) {
        const int t = dir ? s : len - 1 - s;
        const long frame = (long)b * T + t;
        const bool has_prev = s + 1 < len;
        for (int j = tid; j < H; j += GEN_THREADS) {
            const float* gp = gates + frame * 10L * H + (long)dir * 5 * H + j;
            const float gi_ = gp[0], gf = gp[H], gg = gp[2 * H], go = gp[3 * H], c = gp[4 * H];
            const float cprev = has_prev ? gates[(frame + dt) * 10L * H + (long)dir * 5 * H + 4 * H + j] : 0.f;
            const float dht = dhb[j] + dy[frame * 2 * H + dir * H + j];
            const float tc = as_tanh(c);
            const float dct = dcb[j] + dht * go * (1.f - tc * tc);
            const float p_o = dht * tc * go * (1.f - go);
            const float p_i = dct * gg * gi_ * (1.f - gi_);
            const float p_f = dct * cprev * gf * (1.f - gf);
            const float p_g = dct * gi_ * (1.f - gg * gg);
            dcb[j] = dct * gf;
            float* d = dg + (frame * 2 + dir) * 4L * H + j;
            d[0] = p_i; d[H] = p_f; d[2 * H] = p_g; d[3 * H] = p_o;
            gb[j] = p_i; gb[H + j] = p_f; gb[2 * H + j] = p_g; gb[3 * H + j] = p_o;
        }
        __syncthreads();
        rnn_plain_matvec_bwd<4>(wd, gb, H, tid, part);
        __syncthreads();
        for (int k = tid; k < H; k += GEN_THREADS) dhb[k] = (part[k] + part[H + k]) + (part[2 * H + k] + part[3 * H + k]);
        __syncthreads();
    }
}

}  // namespace

extern "C" int as_lstm_bidir_fwd(const float* gi, const int64_t* tokens, int64_t tok_stride, const float* w_hh, const float* b_hh,
                                 const int32_t* lengths, int32_t B, int32_t T, int32_t H, float* y, float* gates, void* stream) {
    AS_TRY(rnn_check_args("as_lstm_bidir_fwd", gi && w_hh && b_hh && lengths && y, B, T));
    AS_REQUIRE(!tokens || T <= 32768, AS_ERR_UNSUPPORTED, "as_lstm_bidir_fwd: T=%d > 32768 with a token table", T);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(B, 2);
    int rc = 0;
    if (!rnn_resident(H, gates != nullptr, tokens != nullptr, &rc, [&](auto h, auto train, auto tok) {
        constexpr int HH = decltype(h)::value;
        hipLaunchKernelGGL((lstm_fwd_kernel<HH, decltype(train)::value, decltype(tok)::value>), grid, dim3(LPU * HH),
                           tokens ? (size_t)T * sizeof(int) : 0, st, gi, tokens, (long)tok_stride, w_hh, b_hh, lengths, T, y, gates);
        return 0;
    })) {   // any other hidden size: the plain kernels
        size_t gshm;
        AS_TRY(rnn_plain_lds("as_lstm_bidir_fwd", H, LSTM_FWD_LDS_PER_UNIT, &gshm));
        rnn_with_flags(gates != nullptr, tokens != nullptr, [&](auto train, auto tok) {
            hipLaunchKernelGGL((lstm_fwd_generic_kernel<decltype(train)::value, decltype(tok)::value>), grid, dim3(GEN_THREADS), gshm, st,
                               gi, tokens, (long)tok_stride, w_hh, b_hh, lengths, T, H, y, gates);
            return 0;
        });
    }
    AS_TRY(rc);
    AS_LAUNCH_CHECK("as_lstm_bidir_fwd");
    return 0;
}

extern "C" int as_lstm_bidir_bwd(const float* dy, const float* gates, const float* w_hh, const int32_t* lengths, int32_t B, int32_t T,
                                 int32_t H, float* dg, void* stream) {
    AS_TRY(rnn_check_args("as_lstm_bidir_bwd", dy && gates && w_hh && lengths && dg, B, T));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(B, 2);
    int rc = 0;
    if (!rnn_resident(H, &rc, [&](auto h) {
        constexpr int HH = decltype(h)::value;
        hipLaunchKernelGGL((lstm_bwd_row_kernel<HH>), grid, dim3(4 * HH), 0, st, dy, gates, w_hh, lengths, T, dg);
        return 0;
    })) {   // any other hidden size: the plain kernel
        size_t gshm;
        AS_TRY(rnn_plain_lds("as_lstm_bidir_bwd", H, LSTM_BWD_LDS_PER_UNIT, &gshm));
        hipLaunchKernelGGL(lstm_bwd_generic_kernel, grid, dim3(GEN_THREADS), gshm, st, dy, gates, w_hh, lengths, T, H, dg);
    }
    AS_TRY(rc);
    AS_LAUNCH_CHECK("as_lstm_bidir_bwd");
    return 0;
}
