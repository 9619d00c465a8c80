// Log-mel spectrogram front end of the acoustic recogniser (reference phoneme_recognition/datasets.py:84-92, 123-132, 47-48 and
// the feature part of collate_fn :258-260) on the device: torchaudio's MelSpectrogram defaults (centred frames, reflect padding,
// one-sided power spectrum, HTK filterbank without normalisation), log(max(., clip)), the mono-to-stereo copy and the -1 padding
// of the collated batch, in one launch from the padded waveforms to the (B, channels, n_mels, T_max) tensor the model reads.
//
//   melspec_kernel   one workgroup of W waves (8; 4 at n_fft 2048) per (utterance, tile of MEL_FRAMES_PER_TILE consecutive frames);
//                    wave w takes the frames w, w + W, ... of the tile, one at a time:
//                      load     the frame's n_fft samples, reflection resolved per sample, times the window, as the n_fft / 2
//                               complex numbers z[n] = x[2n] + i x[2n + 1] of the wave's LDS buffer.  The samples come through
//                               registers: all loads of a frame are issued together, one frame ahead of the FFT that uses
//                               them.  Adjacent frames share n_fft - hop samples; the re-reads are served by the caches
//                      FFT      in place, radix 2, decimation in frequency (log2(n_fft / 2) stages), fp32 on the vector ALU;
//                               the result stands in bit-reversed order
//                      untangle lane p takes the pair (k, n_fft / 2 - k): X[k] = E + W^k O and X[n_fft / 2 - k] = conj(E - W^k O)
//                               come from the same two slots, so both powers go back into those slots (bin n_fft / 2 into the
//                               imaginary half of slot 0) and no second buffer is needed
//                      mel      lane = filter: the sum over the filter's own bin range [lo, hi] (a bin outside it has weight 0 and
//                               adds nothing), then the logarithm, into the tile's [n_mels][frames] LDS image.  The ranges are
//                               found once per workgroup by a scan of the filterbank and the weights inside them are staged in
//                               LDS (triangular filters: at most two per bin; a denser bank than the list holds is read
//                               from memory instead)
//                    and the tile is stored with lanes along t: 16 frames = one 64-byte segment per mel row and plane.
// Twiddles: exp(-2 pi i k / n_fft), k < n_fft / 2, computed once per workgroup in fp64 (sincospi) and rounded to fp32 -- the
// values a host table in float64 would hold; no fast-math sine or cosine anywhere.  log(clip) itself is computed on the host in
// fp64, so that a frame of silence is the correctly rounded log(clip) exactly; every other entry is logf (1 ulp).
// Every wave of a workgroup runs the same frames x stages schedule (a wave whose frame lies past the utterance skips the work,
// not the barriers).  Results depend on the frame's samples alone: repeats, and a row alone or inside a batch, are bit-identical.
#include "as_common.h"

#define MEL_FRAMES_PER_TILE 16   // frames per workgroup; melspec.FRAMES_PER_TILE of the Python side
#define MEL_MAX_FILTERS 128
#define MEL_TILE_PITCH (MEL_FRAMES_PER_TILE + 1)

namespace {

__device__ __forceinline__ float2 mel_cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// power of bin k after the untangling pass: bins below n2 stand bit-reversed in the real halves, bin n2 in slot 0's imaginary half
__device__ __forceinline__ float mel_power(const float2* buf, int k, int n2, int shift) {
    return k < n2 ? buf[__brev((unsigned)k) >> shift].x : buf[0].y;
}

// sum over the bins lo .. hi of weight * power in a fixed order: four interleaved partial sums, then (s0 + s1) + (s2 + s3).
// w points at the weight of bin lo, consecutive bins `stride` apart (LDS: the staged list; memory: a column of the filterbank)
template <bool Staged>
__device__ __forceinline__ float mel_sum(const float* w, int stride, const float2* buf, int lo, int hi, int n2, int shift) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = lo;
    for (; k + 3 <= hi; k += 4, w += 4 * (Staged ? 1 : stride)) {
        const int st = Staged ? 1 : stride;
        s0 = fmaf(w[0], mel_power(buf, k, n2, shift), s0);
        s1 = fmaf(w[st], mel_power(buf, k + 1, n2, shift), s1);
        s2 = fmaf(w[2 * st], mel_power(buf, k + 2, n2, shift), s2);
        s3 = fmaf(w[3 * st], mel_power(buf, k + 3, n2, shift), s3);
    }
    for (; k <= hi; ++k, w += (Staged ? 1 : stride)) s0 = fmaf(w[0], mel_power(buf, k, n2, shift), s0);
    return (s0 + s1) + (s2 + s3);
}

// one pair of samples per register pair: lane l holds the complex points l, l + 64, ... of a frame (PL of them)
template <int PL>
__device__ __forceinline__ void mel_fetch(float (&v)[2 * PL], const float* __restrict__ x, int n_b, int s0, int n2, int lane) {
#pragma unroll
    for (int i = 0; i < PL; ++i) {
        const int n = lane + 64 * i;
#pragma unroll
        for (int j = 0; j < 2; ++j) {   // 32-bit offsets inside the row (the host holds the pitch below 2^30): one address register per load
            int s = s0 + 2 * n + j;
            s = s < 0 ? -s : s;
            s = s >= n_b ? 2 * (n_b - 1) - s : s;
            s = s < 0 ? 0 : (s >= n_b ? n_b - 1 : s);   // never outside the row, whatever the lengths are
            v[2 * i + j] = n < n2 ? x[s] : 0.f;
        }
    }
}

// a non-zero weight at flat index idx of the filterbank widens its filter's bin range (idx < 2^18: the quotient is exact)
__device__ __forceinline__ void mel_mark(float w, int idx, int n_mels, float inv_n_mels, int* k_lo, int* k_hi) {
    if (w != 0.f) {
        const int k = (int)(((float)idx + 0.5f) * inv_n_mels);
        const int m = idx - k * n_mels;
        atomicMin(&k_lo[m], k);
        atomicMax(&k_hi[m], k);
    }
}

// LDS: twiddles [n2] float2 | FFT buffers [WAVES][n2] float2 | tile [n_mels][MEL_TILE_PITCH] float | lo, hi [MEL_MAX_FILTERS] int |
// weight offsets [MEL_MAX_FILTERS + 1] int (the last: their count) | staged weights [w_cap] float
// WAVES waves per workgroup; PL = ceil(n_fft / 2 / 64) complex points per lane and frame.  Up to n_fft 1024 the registers are held
// to 128 (four waves per SIMD), so that two eight-wave workgroups share a CU.
template <int WAVES, int PL>
__global__ __launch_bounds__(WAVES * 64, PL <= 8 ? 4 : 1) void melspec_kernel(const float* __restrict__ wave_in, int64_t wave_pitch,
                                                             const int64_t* __restrict__ n_samples, int n_fft, int log2_n2, int hop,
                                                             const float* __restrict__ window, const float* __restrict__ fbanks,
                                                             int n_mels, float inv_n_mels, float clip, float log_clip, int channels,
                                                             float pad_value, float* __restrict__ out, int64_t T_max,
                                                             int64_t* __restrict__ lengths_out) {
    constexpr int THREADS = WAVES * 64;
    constexpr int NB = PL > 1 ? PL / 2 : 1;   // butterflies per lane and stage
    extern __shared__ __align__(16) unsigned char mel_lds[];
    const int n2 = n_fft >> 1, n_freqs = n2 + 1;
    float2* twd = reinterpret_cast<float2*>(mel_lds);
    float2* bufs = twd + n2;
    float* tile_img = reinterpret_cast<float*>(bufs + WAVES * n2);
    int* k_lo = reinterpret_cast<int*>(tile_img + n_mels * MEL_TILE_PITCH);
    int* k_hi = k_lo + MEL_MAX_FILTERS;
    int* w_off = k_hi + MEL_MAX_FILTERS;
    float* wts = reinterpret_cast<float*>(w_off + MEL_MAX_FILTERS + 1);
    const int w_cap = 2 * n_freqs + 2 * MEL_MAX_FILTERS;

    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int b = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * MEL_FRAMES_PER_TILE;
    int64_t n_b = n_samples[b];
    n_b = n_b < 0 ? 0 : (n_b > wave_pitch ? wave_pitch : n_b);
    int64_t T_b = n_b <= n2 ? 0 : 1 + n_b / hop;   // reflection needs n_b > n_fft / 2: anything shorter is an all-padding row
    T_b = T_b > T_max ? T_max : T_b;
    if (lengths_out && blockIdx.x == 0 && tid == 0) lengths_out[b] = T_b;

    if (t0 < T_b) {   // the same for every thread of the workgroup: a tile of padding alone skips to the store
        const float* x = wave_in + (int64_t)b * wave_pitch;
        float v[2 * PL];   // the wave's next frame, on its way while the scan below and the current frame's FFT run
        bool live = t0 + wv < T_b;      // wave-uniform
        if (live) mel_fetch<PL>(v, x, (int)n_b, (int)((t0 + wv) * hop) - n2, n2, lane);

        for (int k = tid; k < n2; k += THREADS) {
            double s, c;
            sincospi(-2.0 * (double)k / (double)n_fft, &s, &c);
            twd[k] = make_float2((float)c, (float)s);
        }
        if (tid < MEL_MAX_FILTERS) {
            k_lo[tid] = n_freqs;
            k_hi[tid] = -1;
        }
        __syncthreads();
        {   // filter m's bin range [lo, hi]: the filterbank as one flat list, 16 bytes per lane and load, eight loads in flight
            const int total = n_freqs * n_mels, n4 = total >> 2;
            const float4* fb4 = reinterpret_cast<const float4*>(fbanks);
            for (int j0 = tid; j0 < n4; j0 += 8 * THREADS) {
                float4 q[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int j = j0 + u * THREADS;
                    q[u] = j < n4 ? fb4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int idx = 4 * (j0 + u * THREADS);
                    mel_mark(q[u].x, idx, n_mels, inv_n_mels, k_lo, k_hi);
                    mel_mark(q[u].y, idx + 1, n_mels, inv_n_mels, k_lo, k_hi);
                    mel_mark(q[u].z, idx + 2, n_mels, inv_n_mels, k_lo, k_hi);
                    mel_mark(q[u].w, idx + 3, n_mels, inv_n_mels, k_lo, k_hi);
                }
            }
            if (tid < (total & 3)) mel_mark(fbanks[(total & ~3) + tid], (total & ~3) + tid, n_mels, inv_n_mels, k_lo, k_hi);
        }
        float win[2 * PL];   // the lane's window values, the same for every frame (loaded behind the scan: fewer live registers there)
#pragma unroll
        for (int i = 0; i < PL; ++i) {
            const int n = lane + 64 * i;
            const float2 w = n < n2 ? reinterpret_cast<const float2*>(window)[n] : make_float2(0.f, 0.f);
            win[2 * i] = w.x;
            win[2 * i + 1] = w.y;
        }
        __syncthreads();
        if (wv == 0) {   // where filter m's weights start in the staged list: an exclusive scan of the range lengths
            const int c0 = lane < n_mels ? max(0, k_hi[lane] - k_lo[lane] + 1) : 0;
            const int c1 = lane + 64 < n_mels ? max(0, k_hi[lane + 64] - k_lo[lane + 64] + 1) : 0;
            int s0 = c0, s1 = c1;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u0 = __shfl_up(s0, o, 64), u1 = __shfl_up(s1, o, 64);
                if (lane >= o) { s0 += u0; s1 += u1; }
            }
            const int total0 = __shfl(s0, 63, 64);
            w_off[lane] = s0 - c0;
            w_off[lane + 64] = total0 + s1 - c1;
            if (lane == 63) w_off[MEL_MAX_FILTERS] = total0 + s1;
        }
        __syncthreads();
        const bool staged = w_off[MEL_MAX_FILTERS] <= w_cap;   // triangular filters: at most two per bin.  Anything denser stays in memory
        if (staged) {   // staged entry e belongs to the last filter whose offset is <= e (filters without a bin share an offset)
            const int count = w_off[MEL_MAX_FILTERS];
            for (int e = tid; e < count; e += THREADS) {
                int m = 0;
#pragma unroll
                for (int step = MEL_MAX_FILTERS / 2; step > 0; step >>= 1)
                    if (m + step < n_mels && w_off[m + step] <= e) m += step;
                wts[e] = fbanks[(int64_t)(k_lo[m] + e - w_off[m]) * n_mels + m];
            }
        }
        // (the barrier behind the first frame's LDS image orders these writes before the first mel stage too)

        float2* buf = bufs + wv * n2;
        const int shift = 32 - log2_n2;
        for (int fi = wv; fi < MEL_FRAMES_PER_TILE; fi += WAVES) {
            if (live) {
#pragma unroll
                for (int i = 0; i < PL; ++i) {
                    const int n = lane + 64 * i;
                    if (n < n2) buf[n] = make_float2(v[2 * i] * win[2 * i], v[2 * i + 1] * win[2 * i + 1]);
                }
            }
            const bool live_now = live;
            live = fi + WAVES < MEL_FRAMES_PER_TILE && t0 + fi + WAVES < T_b;
            if (live) mel_fetch<PL>(v, x, (int)n_b, (int)((t0 + fi + WAVES) * hop) - n2, n2, lane);
            __syncthreads();
            for (int sh = log2_n2 - 1; sh >= 0; --sh) {   // half = 1 << sh
                if (live_now) {   // a stage's butterflies touch disjoint slots: all operands are read before any result is written
                    const int half = 1 << sh;
                    float2 a[NB], c[NB], tw[NB];
#pragma unroll
                    for (int i = 0; i < NB; ++i) {
                        const int j = lane + 64 * i;
                        const int r = j & (half - 1);
                        const int pos = ((j >> sh) << (sh + 1)) + r;
                        if (j < (n2 >> 1)) {
                            a[i] = buf[pos];
                            c[i] = buf[pos + half];
                            tw[i] = twd[r << (log2_n2 - sh)];   // exp(-2 pi i r / (2 half))
                        }
                    }
#pragma unroll
                    for (int i = 0; i < NB; ++i) {
                        const int j = lane + 64 * i;
                        const int pos = ((j >> sh) << (sh + 1)) + (j & (half - 1));
                        if (j < (n2 >> 1)) {
                            buf[pos] = make_float2(a[i].x + c[i].x, a[i].y + c[i].y);
                            buf[pos + half] = mel_cmul(make_float2(a[i].x - c[i].x, a[i].y - c[i].y), tw[i]);
                        }
                    }
                }
                __syncthreads();
            }
            if (live_now) {
                for (int k = lane; k <= (n2 >> 1); k += 64) {
                    if (k == 0) {
                        const float2 z = buf[0];
                        const float x0 = z.x + z.y, xn = z.x - z.y;
                        buf[0] = make_float2(x0 * x0, xn * xn);
                    } else {
                        const int k2 = n2 - k;
                        const int ia = (int)(__brev((unsigned)k) >> shift), ib = (int)(__brev((unsigned)k2) >> shift);
                        const float2 A = buf[ia], Bz = buf[ib];
                        const float2 E = make_float2(0.5f * (A.x + Bz.x), 0.5f * (A.y - Bz.y));
                        const float2 O = make_float2(0.5f * (A.y + Bz.y), -0.5f * (A.x - Bz.x));
                        const float2 G = mel_cmul(twd[k], O);
                        const float pr = E.x + G.x, pi = E.y + G.y, qr = E.x - G.x, qi = E.y - G.y;
                        buf[ia].x = pr * pr + pi * pi;
                        if (k2 != k) buf[ib].x = qr * qr + qi * qi;
                    }
                }
            }
            __syncthreads();
            if (live_now) {
                for (int m = lane; m < n_mels; m += 64) {
                    const int lo = k_lo[m], hi = k_hi[m];
                    float acc = staged ? mel_sum<true>(wts + w_off[m], 1, buf, lo, hi, n2, shift)
                                       : mel_sum<false>(fbanks + (int64_t)lo * n_mels + m, n_mels, buf, lo, hi, n2, shift);
                    if (clip > 0.f) acc = acc <= clip ? log_clip : logf(acc);   // a NaN power stays NaN, as under torch.clamp
                    tile_img[m * MEL_TILE_PITCH + fi] = acc;
                }
            }
            __syncthreads();   // the tile image is complete after the last round; the buffer is free for the next frame
        }
    }

    // store: lanes along t, 16 frames = 64 bytes per (plane, mel) row
    const int rows = channels * n_mels;
    for (int idx = tid; idx < rows * MEL_FRAMES_PER_TILE; idx += THREADS) {
        const int row = idx / MEL_FRAMES_PER_TILE, fi = idx % MEL_FRAMES_PER_TILE;
        const int64_t t = t0 + fi;
        if (t >= T_max) continue;
        const int m = row % n_mels;
        const float v = t < T_b ? tile_img[m * MEL_TILE_PITCH + fi] : pad_value;
        out[((int64_t)b * rows + row) * T_max + t] = v;
    }
}

}  // namespace

extern "C" int as_melspec_fwd(const float* wave, int64_t wave_pitch, const int64_t* n_samples, int32_t B, int32_t n_fft, int32_t hop,
                              const float* window, const float* fbanks, int32_t n_mels, float clip, int32_t channels,
                              float pad_value, float* out, int64_t T_max, int64_t* lengths_out, void* stream) {
    AS_REQUIRE(wave && n_samples && window && fbanks && out && B >= 1 && wave_pitch >= 1 && T_max >= 1, AS_ERR_BAD_ARG,
               "as_melspec_fwd: bad argument");
    AS_REQUIRE(n_fft >= 64 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0, AS_ERR_UNSUPPORTED,
               "as_melspec_fwd: n_fft must be a power of two in [64, 2048], got %d", n_fft);
    AS_REQUIRE(hop >= 1 && n_mels >= 1 && n_mels <= MEL_MAX_FILTERS && (channels == 1 || channels == 2), AS_ERR_UNSUPPORTED,
               "as_melspec_fwd: hop %d, n_mels %d (1 to %d) or channels %d (1 or 2) not supported", hop, n_mels, MEL_MAX_FILTERS, channels);
    // offsets inside a row are 32-bit, and the reflection forms 2 (n_b - 1) - s: rows stay below 2^30 samples
    AS_REQUIRE(wave_pitch <= 0x3fff0000LL, AS_ERR_UNSUPPORTED, "as_melspec_fwd: rows of %lld samples exceed the 32-bit offsets inside a row",
               (long long)wave_pitch);
    AS_REQUIRE(as_aligned16(window) && as_aligned16(fbanks), AS_ERR_BAD_ARG,
               "as_melspec_fwd: the window and the filterbank must be 16-byte aligned");
    const int64_t tiles = (T_max + MEL_FRAMES_PER_TILE - 1) / MEL_FRAMES_PER_TILE;
    AS_REQUIRE(tiles < 0x7fffffffLL && B <= 65535, AS_ERR_UNSUPPORTED, "as_melspec_fwd: %lld tiles x %d utterances exceed one grid",
               (long long)tiles, B);
    int log2_n2 = 0;
    while ((2 << log2_n2) < n_fft) ++log2_n2;
    const int n2 = n_fft / 2;
    const float log_clip = clip > 0.f ? (float)log((double)clip) : 0.f;
    const float inv_n_mels = 1.0f / (float)n_mels;
    // eight waves, two frames each, while their FFT buffers fit beside the rest in 64 KB of LDS; four waves at n_fft 2048
    as_up_to<1, 2, 4, 8, 16>(as_cdiv(n2, 64), [&](auto per_lane) {
        constexpr int PL = decltype(per_lane)::value;
        constexpr int WAVES = PL == 16 ? 4 : 8;
        const size_t lds = (size_t)n2 * 8 * (1 + WAVES) + (size_t)n_mels * MEL_TILE_PITCH * 4 + (3 * MEL_MAX_FILTERS + 1) * 4 +
                           (size_t)(2 * (n2 + 1) + 2 * MEL_MAX_FILTERS) * 4;   // <= 60 KB
        hipLaunchKernelGGL((melspec_kernel<WAVES, PL>), dim3((unsigned)tiles, (unsigned)B), dim3(WAVES * 64), lds, (hipStream_t)stream,
                           wave, wave_pitch, n_samples, n_fft, log2_n2, hop, window, fbanks, n_mels, inv_n_mels, clip, log_clip,
                           channels, pad_value, out, T_max, lengths_out);
    });
    AS_LAUNCH_CHECK("as_melspec_fwd");
    return 0;
}
