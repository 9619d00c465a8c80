// What the CTC kernels share (ctc.hip: loss and gradient; ctc_align.hip: the Viterbi path): the size limit and the per-utterance
// size check.
#pragma once
#include "as_common.h"

constexpr int CTC_MAX_L = 2047;  // S = 2L + 1 <= 4095 states: 16 per thread of the 256-thread recursion

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
