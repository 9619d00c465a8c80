// Speech from the tube on the device: a glottal source (as_vt_glottal_source) and a time-domain Kelly-Lochbaum waveguide with
// time-varying sections (as_vt_waveguide).  The reference has no acoustic stage, so the definition is THIS PROJECT'S OWN, an
// ASSUMPTION whose parity with any other synthesiser is unpinned; include/artspeech_hip.h states it in full (the conventions,
// the noise, the source, the ladder, the status bits) and this file follows it symbol for symbol.  All arithmetic is float64.
//
// vts_source_kernel: grid (B, G), 256 threads.  The phase is linear within a frame, so a scan over the frames' totals plus a
// closed form per sample gives it: every workgroup walks the frames in chunks of 64, wave 0 scans the chunk's totals (a wave
// scan in a fixed order plus the carry of the chunks before) and leaves base, f0 and its slope per frame in LDS; workgroup g
// then writes the samples of the chunks c with c % G == g, one sample per thread and pass.  No scan over samples, no atomics.
//
// vtw_kernel: the hot path, ~10^5 dependent steps per utterance.  One wave per utterance, one launch per batch; lane i owns
// section i and keeps R_i and L_i in registers.
//   - the two neighbour reads of a step are DPP wave shifts (v_mov_b32 wave_shr:1 / wave_shl:1 on the two halves of a double).
//     The lane without a neighbour keeps the shift's `old` operand: lane 0 gets source + r_g L_0 there, so the glottis end
//     costs no select; the lips end is one select on a loop-invariant mask;
//   - lane j holds k_j and, again, k_{j-1} (formed from the same two areas by the same expression: equal bits), so both new
//     waves of a lane come from values shifted at the top of the step and no second shift sits behind the multiply;
//   - the reflection coefficients of frame t' and the areas of the frame after it are formed / loaded when frame t begins, a
//     frame ahead of their use; per sample k = fma(dk, s / S, k_t);
//   - source, s / S and the frication term are staged 64 samples at a time, one per lane (the raw loads are issued a batch
//     ahead), and read per sample with v_readlane at the wave-uniform sample index; R_{K-1} of sample i is kept by lane i (one compare, two selects) and
//     64 outputs leave in one coalesced store, differenced there;
//   - nothing on the per-sample chain waits on global memory or LDS (there is no LDS), no scratch, no atomics: two launches
//     give equal bits, an utterance alone or in a batch gives equal bits.
// Time is not split across workgroups: that needs a scan over products of 2K x 2K operators.
// A pass before the recurrence looks at every used area, source sample and gain: a non-finite one makes the utterance NaN.
#include <math.h>

#include <vector>

#include "as_common.h"
#include "as_device.h"

namespace {

constexpr int VTW_MAX_K = 64;   // one lane per section
constexpr int VTS_THREADS = 256;
constexpr int VTS_MAX_GROUPS = 16;

// nu(seed, stream, b, n) in [-1, 1): the splitmix64 finaliser of dropout_scale (rowops.hip) on ((2 b + stream) << 40) | n
__device__ __forceinline__ double vts_noise(unsigned long long seed, int stream, int b, unsigned long long n) {
    const unsigned long long idx = ((unsigned long long)(2 * b + stream) << 40) | n;
    unsigned long long z = seed + (idx + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double u = (double)(z >> 11) * (1.0 / 9007199254740992.0);   // 53 random bits -> [0, 1), exact
    return 2.0 * u - 1.0;
}

// ---- the source

struct VtsArgs {
    const double* f0;
    const double* voiced;
    const double* asp;
    const int* frames;
    int T, S;
    double fs, rise, fall;
    unsigned long long seed;
    double* source;
    long pitch;
    int* status;
};

__global__ __launch_bounds__(VTS_THREADS) void vts_source_kernel(VtsArgs a) {
    __shared__ double s_base[64], s_g[64], s_d[64];
    __shared__ double s_carry;
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
    const int F = as_clamp_length(a.frames[b], a.T), S = a.S;
    const long nb = (long)F * S;
    const double* f0 = a.f0 + (long)b * a.T;
    const double* va = a.voiced + (long)b * a.T;
    const double* as = a.asp + (long)b * a.T;
    double* out = a.source + (long)b * a.pitch;
    const long step = (long)gridDim.y * VTS_THREADS, first = (long)blockIdx.y * VTS_THREADS + tid;
    for (long n = nb + first; n < a.pitch; n += step) out[n] = 0.0;
    int bad = 0;
    for (int t = tid; t < F; t += VTS_THREADS) bad |= !(isfinite(f0[t]) && isfinite(va[t]) && isfinite(as[t]));
    bad = __syncthreads_or(bad);
    if (blockIdx.y == 0 && tid == 0 && a.status) a.status[b] = bad ? 2 : 0;
    if (bad) {
        for (long n = first; n < nb; n += step) out[n] = NAN;
        return;
    }
    if (tid == 0) s_carry = 0.0;
    const double dS = (double)S;
    for (int c = 0, t0 = 0; t0 < F; ++c, t0 += 64) {   // workgroup-uniform
        __syncthreads();   // the chunk before is read, s_carry is set
        if (tid < 64) {
            const int t = t0 + lane;
            double g = 0.0, d = 0.0, total = 0.0;
            if (t < F) {
                const int tn = t + 1 < F ? t + 1 : F - 1;
                g = fmax(f0[t], 0.0);
                d = fmax(f0[tn], 0.0) - g;
                total = (g * dS + d * ((dS - 1.0) * 0.5)) / a.fs;   // sum over the frame's S samples, in cycles
            }
            const double incl = as_wave_scan(total, lane, AsAdd{});
            double excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 0.0;
            const double carry = s_carry;
            s_base[lane] = carry + excl;
            s_g[lane] = g;
            s_d[lane] = d;
            const double next = carry + __shfl(incl, 63, 64);
            if (lane == 0) s_carry = next;   // read above by this very wave, in program order
        }
        __syncthreads();
        if (c % (int)gridDim.y != (int)blockIdx.y) continue;
        const int used = F - t0 < 64 ? F - t0 : 64;
        for (int i = tid; i < used * S; i += VTS_THREADS) {
            const int j = i / S, s = i - j * S, t = t0 + j;
            const int tn = t + 1 < F ? t + 1 : F - 1;
            const double ds = (double)s, frac = ds / dS;
            const double within = s_g[j] * ds + s_d[j] * ((ds * (ds - 1.0) * 0.5) / dS);
            const double phase = s_base[j] + within / a.fs;
            const double th = phase - floor(phase);
            double pulse = 0.0;
            if (th < a.rise) pulse = 0.5 * (1.0 - cos(M_PI * th / a.rise));
            else if (th < a.rise + a.fall) pulse = cos(M_PI * (th - a.rise) / (2.0 * a.fall));
            const long n = (long)t * S + s;
            const double v = va[t] + (va[tn] - va[t]) * frac, h = as[t] + (as[tn] - as[t]) * frac;
            out[n] = v * pulse + h * vts_noise(a.seed, 0, b, (unsigned long long)n);
        }
    }
}

// ---- the ladder

struct VtwArgs {
    const double* areas;
    long a_utt, a_frame, a_sec;
    const int* sections;
    const int* frames;
    int T, S;
    const double* source;
    const int* inj;
    const double* gain;
    unsigned long long seed;
    double r_g, r_l, mu, min_area;
    int radiation;
    double* out64;
    float* out32;
    long pitch;
    int* status;
};

// v of the lane that the DPP control selects; a lane whose source lane does not exist keeps `old`
template <int CTRL>
__device__ __forceinline__ double vtw_shift(double old, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// the same, a lane without a source lane reads 0
template <int CTRL>
__device__ __forceinline__ double vtw_shift_zero(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
constexpr int VTW_SHL1 = 0x130, VTW_SHR1 = 0x138;   // wave_shl:1: lane i reads lane i + 1; wave_shr:1: lane i reads lane i - 1
// v of lane `i`, i wave-uniform
__device__ __forceinline__ double vtw_read(double v, int i) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), i), __builtin_amdgcn_readlane(__double2loint(v), i));
}
// the three areas a lane needs of one frame, as loaded
struct VtwAreas {
    double below, own, above;   // A_{j-1}, A_j, A_{j+1}, the index held inside [0, K - 1]
};

template <bool INJECT>
__global__ __launch_bounds__(64) void vtw_kernel(VtwArgs a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int K = a.sections[b], S = a.S;
    const int F = as_clamp_length(a.frames[b], a.T);
    const int nb = F * S;   // the host has checked T S < 2^31
    double* o64 = a.out64 ? a.out64 + (long)b * a.pitch : nullptr;
    float* o32 = a.out32 ? a.out32 + (long)b * a.pitch : nullptr;
    const double* src = a.source + (long)b * a.pitch;
    const double* ar = a.areas + (long)b * a.a_utt;
    const int* inj = INJECT ? a.inj + (long)b * a.T : nullptr;
    const double* gain = INJECT ? a.gain + (long)b * a.T : nullptr;

    for (long n = (long)nb + lane; n < a.pitch; n += 64) {
        if (o64) o64[n] = 0.0;
        if (o32) o32[n] = 0.f;
    }
    // the pass before the recurrence: status
    int bad = 0, closed = 0;
    for (int i = lane; i < F * K; i += 64) {   // F K <= T Kmax, an int (checked)
        const int t = i / K, j = i - t * K;
        const double A = ar[t * a.a_frame + j * a.a_sec];
        if (!(isfinite(A) && A > 0.0)) bad = 1;
        else if (A < a.min_area) closed = 1;
    }
    for (int n = lane; n < nb; n += 64) bad |= !isfinite(src[n]);
    if (INJECT)
        for (int t = lane; t < F; t += 64) bad |= !isfinite(gain[t]);
    bad = __any(bad);
    closed = __any(closed);
    if (lane == 0 && a.status) a.status[b] = (closed ? 1 : 0) | (bad ? 2 : 0);
    if (bad) {
        for (int n = lane; n < nb; n += 64) {
            if (o64) o64[n] = NAN;
            if (o32) o32[n] = NAN;
        }
        return;
    }
    if (nb == 0) return;

    const int jb = lane >= 1 ? (lane - 1 < K ? lane - 1 : K - 1) : 0, jo = lane < K ? lane : K - 1, ja = lane + 1 < K ? lane + 1 : K - 1;
    const bool has_k = lane < K - 1, has_kp = lane >= 1 && lane < K, lips = lane == K - 1;
    auto load_frame = [&](int t) {
        const double* p = ar + t * a.a_frame;
        return VtwAreas{p[jb * a.a_sec], p[jo * a.a_sec], p[ja * a.a_sec]};
    };
    auto refl = [&](double x, double y) {   // (A_j - A_{j+1}) / (A_j + A_{j+1}) of the clamped areas
        x = x < a.min_area ? a.min_area : x;
        y = y < a.min_area ? a.min_area : y;
        return (x - y) / (x + y);
    };
    // what a batch of 64 samples stages, one sample per lane: the raw loads, issued a batch ahead
    struct Raw {
        double src, g0, g1;
        int sec;
    };
    auto load_batch = [&](int n0) {   // a lane past the end reads the last sample again: no branch, so a load's target is the
        Raw r{0.0, 0.0, 0.0, -1};     // register that waits for the next batch, and nothing has to wait for the load to copy it
        const int n = n0 + lane < nb ? n0 + lane : nb - 1;
        r.src = src[n];
        if (INJECT) {
            const int t = n / S, tn = t + 1 < F ? t + 1 : F - 1;
            r.sec = inj[t];
            r.g0 = gain[t];
            r.g1 = gain[tn];
        }
        return r;
    };

    VtwAreas pend = load_frame(0);
    double kB = has_k ? refl(pend.own, pend.above) : 0.0, kpB = has_kp ? refl(pend.below, pend.own) : 0.0;
    pend = load_frame(F > 1 ? 1 : 0);
    const double dS = (double)S, gain_out = 1.0 + a.r_l;
    // the staged values of a batch, one sample per lane, from the raw loads of a batch ago
    Raw raw = load_batch(0);
    double st_src = 0.0, st_frac = 0.0, st_e = 0.0;
    int st_sec = -1;
    auto stage = [&](int n0) {
        const int nl = n0 + lane;
        st_src = raw.src;
        st_frac = (double)(nl % S) / dS;
        if (INJECT) {
            st_sec = raw.sec;
            st_e = 0.0;
            if (st_sec >= 0 && nl < nb) st_e = (raw.g0 + (raw.g1 - raw.g0) * st_frac) * vts_noise(a.seed, 1, b, (unsigned long long)nl);
        }
    };
    double kA = 0.0, kpA = 0.0, dk = 0.0, dkp = 0.0, R = 0.0, L = 0.0, y_last = 0.0;
    int s = 0, t = -1;   // wave-uniform: the next sample's place in its frame, the frame of the sample before
    for (int n0 = 0; n0 < nb; n0 += 64) {
        stage(n0);
        asm volatile("" ::"v"(st_src));   // the one wait for a batch's loads is here, a batch after they were issued
        raw = load_batch(n0 + 64);
        const int m = nb - n0 < 64 ? nb - n0 : 64;
        double col = 0.0;
        for (int i = 0; i < m;) {
            if (s == 0) {   // frame t + 1 begins: its k and the next frame's are at hand, the frame after that is requested
                ++t;
                kA = kB;
                kpA = kpB;
                kB = has_k ? refl(pend.own, pend.above) : 0.0;
                kpB = has_kp ? refl(pend.below, pend.own) : 0.0;
                dk = kB - kA;
                dkp = kpB - kpA;
                pend = load_frame(t + 2 < F ? t + 2 : F - 1);
            }
            const int run = S - s < m - i ? S - s : m - i;   // to the end of the frame or of the batch, whichever comes first
            for (const int end = i + run; i < end; ++i) {   // the recurrence: everything below is registers
                const double sv = vtw_read(st_src, i), fv = vtw_read(st_frac, i), r_lips = vtw_read(R, K - 1);
                col = lane == i ? r_lips : col;                               // R_{K-1} of this sample, kept by lane i
                const double r_in = vtw_shift<VTW_SHR1>(a.r_g * L + sv, R);   // R_{j-1}; lane 0: source + r_g L_0
                const double l_up = vtw_shift_zero<VTW_SHL1>(L);              // L_{j+1}
                const double l_in = lips ? a.r_l * R : l_up;
                const double k = dk * fv + kA, kp = dkp * fv + kpA;           // 0 where the lane has no junction
                double r_new = r_in + kp * (r_in - L);
                if (INJECT) {
                    const int sec = __builtin_amdgcn_readlane(st_sec, i);
                    const double e = vtw_read(st_e, i);
                    r_new += lane == sec ? e : 0.0;
                }
                L = a.mu * (l_in + k * (R - l_in));
                R = a.mu * r_new;
            }
            s = s + run == S ? 0 : s + run;
        }
        double y = gain_out * col;   // 64 outputs in one store
        if (a.radiation) {
            const double before = vtw_shift<VTW_SHR1>(y_last, y);
            y_last = vtw_read(y, 63);
            y -= before;
        }
        if (lane < m) {
            if (o64) o64[n0 + lane] = y;
            if (o32) o32[n0 + lane] = (float)y;
        }
    }
}

}  // namespace

extern "C" int as_vt_glottal_source(const double* f0, const double* voiced_amp, const double* asp_amp, const int32_t* frames,
                                    int32_t B, int32_t T, int32_t S, double sample_rate, uint64_t seed, double rise, double fall,
                                    double* source, int64_t pitch, int32_t* status, void* stream) {
    AS_REQUIRE(B >= 0 && T >= 0 && S >= 1 && S <= (1 << 24) && (int64_t)T * S <= 0x7fffffff, AS_ERR_BAD_ARG,
               "as_vt_glottal_source: B = %d, T = %d, S = %d (B, T >= 0, 1 <= S <= 2^24, T S < 2^31)", B, T, S);
    AS_REQUIRE(pitch >= (int64_t)T * S, AS_ERR_BAD_ARG, "as_vt_glottal_source: a row pitch of %lld for T S = %lld samples",
               (long long)pitch, (long long)T * S);
    AS_REQUIRE(sample_rate > 0.0 && isfinite(sample_rate) && rise > 0.0 && fall > 0.0 && rise + fall <= 1.0, AS_ERR_BAD_ARG,
               "as_vt_glottal_source: sample_rate %g, rise %g, fall %g (all positive, rise + fall <= 1)", sample_rate, rise, fall);
    if (B == 0) return 0;
    AS_REQUIRE(f0 && voiced_amp && asp_amp && frames && source, AS_ERR_BAD_ARG, "as_vt_glottal_source: a required pointer is NULL");
    VtsArgs a;
    a.f0 = f0;
    a.voiced = voiced_amp;
    a.asp = asp_amp;
    a.frames = frames;
    a.T = T;
    a.S = S;
    a.fs = sample_rate;
    a.rise = rise;
    a.fall = fall;
    a.seed = seed;
    a.source = source;
    a.pitch = (long)pitch;
    a.status = status;
    int groups = as_cdiv(T, 64);
    groups = groups < 1 ? 1 : (groups > VTS_MAX_GROUPS ? VTS_MAX_GROUPS : groups);
    hipLaunchKernelGGL(vts_source_kernel, dim3((unsigned)B, (unsigned)groups), dim3(VTS_THREADS), 0, (hipStream_t)stream, a);
    AS_LAUNCH_CHECK("as_vt_glottal_source");
    return 0;
}

extern "C" int as_vt_waveguide(const double* areas, int64_t a_utt, int64_t a_frame, int64_t a_sec, const int32_t* sections,
                               const int32_t* frames, int32_t B, int32_t T, int32_t Kmax, int32_t S, const double* source,
                               const int32_t* inject_section, const double* inject_gain, uint64_t seed, double r_g, double r_l,
                               double mu, double min_area, int32_t radiation, double* out64, float* out32, int64_t pitch,
                               int32_t* status, void* stream) {
    AS_REQUIRE(B >= 0 && T >= 0 && S >= 1 && S <= (1 << 24) && (int64_t)T * S <= 0x7fffffff, AS_ERR_BAD_ARG,
               "as_vt_waveguide: B = %d, T = %d, S = %d (B, T >= 0, 1 <= S <= 2^24, T S < 2^31)", B, T, S);
    AS_REQUIRE(Kmax >= 1 && (int64_t)T * Kmax <= 0x7fffffff, AS_ERR_BAD_ARG, "as_vt_waveguide: Kmax = %d with T = %d", Kmax, T);
    AS_REQUIRE(pitch >= (int64_t)T * S, AS_ERR_BAD_ARG, "as_vt_waveguide: a row pitch of %lld for T S = %lld samples", (long long)pitch,
               (long long)T * S);
    AS_REQUIRE(isfinite(r_g) && isfinite(r_l) && isfinite(mu) && min_area > 0.0 && isfinite(min_area), AS_ERR_BAD_ARG,
               "as_vt_waveguide: r_g %g, r_l %g, mu %g, min_area %g (finite, min_area > 0)", r_g, r_l, mu, min_area);
    AS_REQUIRE(radiation == 0 || radiation == 1, AS_ERR_BAD_ARG, "as_vt_waveguide: radiation %d (0 = none, 1 = difference)", radiation);
    AS_REQUIRE((inject_section == nullptr) == (inject_gain == nullptr), AS_ERR_BAD_ARG,
               "as_vt_waveguide: inject_section and inject_gain come together");
    if (B == 0) return 0;
    AS_REQUIRE(areas && sections && frames && source, AS_ERR_BAD_ARG, "as_vt_waveguide: a required pointer is NULL");
    // The section counts and the injection sections decide what is refused, so they are read back before the launch: one
    // copy of B (1 + T) integers on `stream`, waited for.  Nothing is truncated and nothing is launched on a refusal.
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> ks((size_t)B), nf((size_t)B), sec(inject_section ? (size_t)B * T : 0);
    hipError_t e = hipMemcpyAsync(ks.data(), sections, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nf.data(), frames, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !sec.empty()) e = hipMemcpyAsync(sec.data(), inject_section, sizeof(int32_t) * sec.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    AS_REQUIRE(e == hipSuccess, (int)e, "as_vt_waveguide: reading the section counts back failed: %s", hipGetErrorString(e));
    for (int b = 0; b < B; ++b) {
        AS_REQUIRE(ks[b] >= 1 && ks[b] <= VTW_MAX_K, AS_ERR_UNSUPPORTED, "as_vt_waveguide: utterance %d has %d sections (1 .. %d supported)",
                   b, ks[b], VTW_MAX_K);
        AS_REQUIRE(ks[b] <= Kmax, AS_ERR_BAD_ARG, "as_vt_waveguide: utterance %d has %d sections, the rows hold %d", b, ks[b], Kmax);
        const int used = nf[b] < 0 ? 0 : (nf[b] > T ? T : nf[b]);
        for (int t = 0; !sec.empty() && t < used; ++t) {
            const int j = sec[(size_t)b * T + t];
            AS_REQUIRE(j == -1 || (j >= 1 && j <= ks[b] - 1), AS_ERR_BAD_ARG,
                       "as_vt_waveguide: utterance %d, frame %d injects at section %d (1 .. %d, or -1 for none)", b, t, j, ks[b] - 1);
        }
    }
    VtwArgs a;
    a.areas = areas;
    a.a_utt = (long)a_utt;
    a.a_frame = (long)a_frame;
    a.a_sec = (long)a_sec;
    a.sections = sections;
    a.frames = frames;
    a.T = T;
    a.S = S;
    a.source = source;
    a.inj = inject_section;
    a.gain = inject_gain;
    a.seed = seed;
    a.r_g = r_g;
    a.r_l = r_l;
    a.mu = mu;
    a.min_area = min_area;
    a.radiation = radiation;
    a.out64 = out64;
    a.out32 = out32;
    a.pitch = (long)pitch;
    a.status = status;
    as_flag(inject_section != nullptr, [&](auto inject) {
        hipLaunchKernelGGL(vtw_kernel<decltype(inject)::value>, dim3((unsigned)B), dim3(64), 0, st, a);
    });
    AS_LAUNCH_CHECK("as_vt_waveguide");
    return 0;
}
