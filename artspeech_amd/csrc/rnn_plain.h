// What the recurrences of gru.hip and lstm.hip share outside their register-resident kernels: the backward mat-vec and the
// padded-frame zeroing of the plain kernels, written once over the gate count NG (GRU 3, LSTM 4), those kernels' LDS sizes,
// and the host's dispatch.
// The plain kernels serve the hidden sizes the register-resident ones are not built for (those hold W_hh in 96 / 128 VGPRs per
// lane at H = 128; at H = 256 it would be twice that): one workgroup of GEN_THREADS threads per (utterance, direction), the
// recurrent state in LDS, W_hh streamed from L2 every step (768 KB per step and workgroup for the GRU at H = 256).  Same
// layouts and packed-sequence semantics as the register-resident kernels; the reduction order over k differs from theirs in
// the last bits.  Several times slower per step -- a correct fallback, not a tuned path (measured: DESIGN.md 8).
#pragma once
#include "as_common.h"
#include "as_device.h"

constexpr int GEN_THREADS = 1024;

// Dynamic LDS of each plain kernel in floats per hidden unit; the launchers size the allocation and word their refusal from these
constexpr int GRU_FWD_LDS_PER_UNIT = 2;     // h double buffer [2][H]
constexpr int GRU_BWD_LDS_PER_UNIT = 9;     // g [3H], dh carried [H], dht * z [H], partial sums [4][H]
constexpr int LSTM_FWD_LDS_PER_UNIT = 3;    // h double buffer [2][H], c [H]
constexpr int LSTM_BWD_LDS_PER_UNIT = 10;   // p [4H], dh carried [H], dc carried [H], partial sums [4][H]
constexpr size_t RNN_PLAIN_LDS_MAX = 64 * 1024;   // no attribute is asked for: the default limit of dynamic LDS

// Backward mat-vec W_hh^T . g over the NG * H gate gradients gb (LDS).  The gate rows are dealt over four thread groups
// (kq = tid >> 8 takes rows kq, kq + 4, ..., eight of them in flight); lanes are consecutive hidden columns (a wave reads 256
// consecutive bytes of a row), 256 columns per pass.  part[kq * H + k]: the group's partial sum for column k; after a barrier
// the caller adds them in a fixed order, (p0 + p1) + (p2 + p3).
template <int NG>
__device__ __forceinline__ void rnn_plain_matvec_bwd(const float* __restrict__ wd, const float* gb, int H, int tid, float* part) {
    const int kq = tid >> 8, kl = tid & 255;   // row group (0..3), column within a block of 256
    for (int k0 = 0; k0 < H; k0 += 256) {
        const int k = k0 + kl;
        const int kc = k < H ? k : H - 1;
        float acc = 0.f;
        for (int i0 = kq; i0 < NG * H; i0 += 32) {
            float wv[8], gv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + 4 * u;
                const int ic = i < NG * H ? i : NG * H - 1;
                wv[u] = wd[(long)ic * H + kc];
                gv[u] = i < NG * H ? gb[ic] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += gv[u] * wv[u];
        }
        if (k < H) part[kq * H + k] = acc;
    }
}

// Exact zeros at the padded frames len .. T - 1 of utterance b of the gate-gradient arrays (they feed time-batched GEMMs over
// all frames): `width` floats per frame at [(b * T + t) * stride + off ...], stride = floats per frame of an array, off = this
// direction's offset in a frame.  out2: a second array of the same layout, or null.
__device__ __forceinline__ void rnn_plain_zero_padded(float* __restrict__ out, float* __restrict__ out2, int b, int T, int len, int width,
                                                      long stride, long off, int tid) {
    for (long i = (long)len * width + tid; i < (long)T * width; i += GEN_THREADS) {
        const long o = ((long)b * T + i / width) * stride + off + i % width;
        out[o] = 0.f;
        if (out2) out2[o] = 0.f;
    }
}

// ---- host
// The checks every recurrence entry shares; `name` is the entry's name in the message
static inline int rnn_check_args(const char* name, bool pointers, int B, int T) {
    AS_REQUIRE(pointers, AS_ERR_BAD_ARG, "%s: null pointer", name);
    AS_REQUIRE(B > 0 && T > 0, AS_ERR_BAD_ARG, "%s: B=%d T=%d", name, B, T);
    return 0;
}
// Dynamic LDS of a plain kernel, or the refusal of a hidden size it cannot serve (the message names the largest it can)
static inline int rnn_plain_lds(const char* name, int H, int floats_per_unit, size_t* bytes) {
    *bytes = (size_t)floats_per_unit * H * sizeof(float);
    AS_REQUIRE(H > 0 && H % 4 == 0 && *bytes <= RNN_PLAIN_LDS_MAX, AS_ERR_UNSUPPORTED, "%s: hidden size %d (a multiple of 4 up to %d)", name, H,
               (int)(RNN_PLAIN_LDS_MAX / (floats_per_unit * sizeof(float)) / 4 * 4));
    return 0;
}
// Runtime choices as compile-time constants for a generic lambda that launches and returns a status code: f(IC<a>, IC<b>) for
// two flags (gates saved, token table); for a register-resident hidden size f(IC<H>) or f(IC<H>, IC<a>, IC<b>), its result in
// *rc, true.  false: not a register-resident size, f was not called and the caller takes its plain kernel.
template <typename F>
int rnn_with_flags(bool a, bool b, F&& f) {
    return as_flag(a, [&](auto fa) { return as_flag(b, [&](auto fb) { return f(fa, fb); }); });
}
template <typename F>
bool rnn_resident(int H, int* rc, F&& f) {
    return as_exactly<32, 64, 128>(H, rc, f);
}
template <typename F>
bool rnn_resident(int H, bool a, bool b, int* rc, F&& f) {
    return rnn_resident(H, rc, [&](auto h) { return rnn_with_flags(a, b, [&](auto fa, auto fb) { return f(h, fa, fb); }); });
}
