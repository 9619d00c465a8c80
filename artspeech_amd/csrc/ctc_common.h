// What the CTC kernels share (ctc.hip: loss and gradient; ctc_align.hip: the Viterbi path): the size limit, the host's argument
// check and choice of the recursion's thread layout, and the per-utterance size check.
#pragma once
#include "as_common.h"

constexpr int CTC_MAX_L = 2047;  // S = 2L + 1 <= 4095 states: 16 per thread of the 256-thread recursion

// The arguments every CTC entry point takes.  `own` is what the entry point adds to the first refusal (its workspace or output
// pointer, the alignment's tgt_stride >= 0); its workspace size and frame limit it checks itself, after this.
static inline int ctc_check(const char* who, const float* x, int32_t T, int32_t B, int32_t C, const int64_t* targets,
                            const int64_t* in_len, const int64_t* tgt_len, int32_t maxL, int32_t blank, bool own) {
    AS_REQUIRE(x && in_len && tgt_len && own && T > 0 && B > 0 && C > 0 && maxL >= 0 && blank >= 0 && blank < C, AS_ERR_BAD_ARG,
               "%s: bad argument", who);
    AS_REQUIRE(targets || maxL == 0, AS_ERR_BAD_ARG, "%s: null targets", who);
    AS_REQUIRE(maxL <= CTC_MAX_L, AS_ERR_UNSUPPORTED, "%s: target length %d (at most %d supported)", who, maxL, CTC_MAX_L);
    return 0;
}
// The recursion's layout for S = 2 maxL + 1 states: f(IC<64>, IC<4>), one wave with 4 states per thread (S <= 256, the exchange
// is a lane shift), else f(IC<256>, IC<16>); f's result
template <typename F>
auto ctc_layout(int maxL, F&& f) {
    if (2 * maxL + 1 <= 64 * 4) return f(IC<64>{}, IC<4>{});
    return f(IC<256>{}, IC<16>{});
}

// validated per-utterance sizes (false: inconsistent lengths; the caller writes NaN instead of reading out of bounds)
__device__ __forceinline__ bool ctc_sizes(const int64_t* in_len, const int64_t* tgt_len, const int64_t* targets, int64_t tgt_stride,
                                          int b, int T, int maxL, int& L, int& Tb, long& toff) {
    const long l = tgt_len[b], tb = in_len[b];
    if (l < 0 || l > maxL || tb < 0 || tb > T) return false;
    L = (int)l;
    Tb = (int)tb;
    if (tgt_stride > 0) {
        toff = (long)b * tgt_stride;
    } else {   // torch's concatenated 1-D form
        long o = 0;
        for (int i = 0; i < b; ++i) o += tgt_len[i];
        toff = o;
    }
    (void)targets;
    return true;
}
