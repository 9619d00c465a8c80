// Vocal-tract acoustics on the device: the volume-velocity transfer function and the formants of every frame of a batch, from the
// frame's tube sections (areas and lengths, as the area function gives them), in one launch.  The reference has no acoustic
// stage -- its area_function.py is imported by nothing -- so the definition below is THIS PROJECT'S OWN and its parity with any
// other synthesiser is unpinned: an ASSUMPTION, like the contour smoothing and the vocal-tract tube.  Unlike those two it has
// closed-form answers: a uniform tube closed at the glottis resonates at (2n - 1) c / 4L, two tubes at the roots of
// tan(k l_1) tan(k l_2) = A_2 / A_1 (tests/test_vt_acoustics_host.py).
//
// Per frame, K sections ordered glottis -> lips, area A_i (cm^2) and length l_i (cm), float64; with `counts` frame n uses its
// first counts[n] sections (a count above K reads K).  Frequencies f_j = f0 + j df, j = 0 .. F-1.  Lossless walls:
//   chain      k = 2 pi f / c, z_i = rho c / A_i, M_i = [[cos k l_i, j z_i sin k l_i], [j sin(k l_i) / z_i, cos k l_i]],
//              [[A, B], [C, D]] = M_1 M_2 ... M_K, the glottis on the left
//   radiation  0: an ideal open end, Z = 0.  1: Flanagan's piston in a baffle on the last section, a = sqrt(A_K / pi),
//              ka = 2 pi f a / c, Z = (rho c / A_K) ((ka)^2 / 2 + j 8 ka / (3 pi))
//   outputs    den = C Z + D and the transfer function H = U_lips / U_glottis = 1 / den, per (frame, bin)
//   formants   on g(f) = |den(f)|^2 (with radiation 0 the poles are zeros of g: no infinity is formed).  Bin j in 1 .. F-2 is a
//              coarse minimum when g_j < g_{j-1} and g_j <= g_{j+1}; they are taken in increasing j, the first n_formants kept.
//              Each is refined in R rounds: the bracket starts as [f_{j-1}, f_{j+1}]; g is evaluated at lo + (hi - lo) m / 65,
//              m = 1 .. 64; the lowest value wins, among equals the lowest m; the new bracket is that point +- (hi - lo) / 65.
//              The formant is the last bracket's midpoint -- the last winner itself, f_j without rounds -- (the bracket is
//              2 df (2 / 65)^R wide), its level -10 log10 g there, the value that won.  Slots that were not found hold NaN.
//   status     bit 0: some used A_i < min_area -- a closure, as in a stop consonant: that area is computed as min_area; not an
//              error.  bit 1: a non-finite area or length, a length <= 0 or counts[n] < 1: every output of the frame is NaN and
//              found = 0.
// Left out on purpose: wall, viscous and heat losses, formant bandwidths, a nasal branch, a time-domain waveform.
//
// The matrices M_i have real diagonals and imaginary off-diagonals, and so has every product of them: A and D stay real, B = j b
// and C = j c_ stay imaginary.  den needs the bottom row alone, two real numbers per frequency:
//   c_ <- c_ cos + d (sin / z_i),   d <- d cos - c_ (z_i sin),   from (0, 1);   den = (d - c_ Im Z) + j c_ Re Z.
//
// vta_kernel: one workgroup of eight waves per frame, (3 K + F) doubles of LDS (5.6 KiB at K = 99, F = 500; 56 KiB at the limits).
//   1. staging: (z_i, 1 / z_i) and l_i go to LDS once; the closure clamp, the non-finite scan and the test whether all the
//      frame's lengths are equal happen here (three workgroup votes, which are also the barrier behind the staging);
//   2. bins: lanes own the bins j in passes of 512; each walks the sections with its two running values in registers, the
//      section constants come as LDS broadcasts, nothing crosses lanes.  den and H are stored, g_j goes to LDS;
//   3. coarse minima: wave 0 walks the bins in order, 64 at a time: a ballot and a prefix count of the lanes below give every
//      minimum its slot; no atomics;
//   4. refinement: wave w takes the formants w, w + 8, ...: per round its 64 lanes are the 64 probes, a shuffle butterfly on
//      (g, m) picks the winner, whose frequency and g are the formant and its level after the last round.
// Two paths through the section walk, chosen per frame (workgroup-uniform): when all used lengths of the frame are equal -- as
// after evenly_spaced_fx, or any tube cut into equal slices -- one sine/cosine pair per frequency serves every section;
// otherwise a pair per (frequency, section).  The equal-length path feeds the same argument k l to the same sincos, so the two
// paths give equal bits on equal inputs.  Everything is float64; no atomics, every choice in a fixed order: two launches give
// equal bits, and a frame alone or inside a batch gives equal bits.
#include <math.h>

#include "as_common.h"
#include "as_device.h"

namespace {

constexpr int VTA_WAVES = 8;
constexpr int VTA_THREADS = VTA_WAVES * 64;
constexpr int VTA_MAX_K = 1024;   // the area function's own limit
constexpr int VTA_MAX_F = 4096;
constexpr int VTA_MAX_FORMANTS = 8;
constexpr int VTA_MAX_ROUNDS = 6;
constexpr int VTA_PROBES = 64;    // one per lane

struct VtaArgs {
    const double* areas;
    long a_frame, a_sec;
    const double* lengths;
    long l_frame, l_sec;
    const int* counts;
    int K, F, radiation, n_formants, rounds;
    double f0, df, c, rho, min_area;
    double* den;
    double* transfer;
    double* freq;
    double* level;
    int* found;
    int* status;
};

// what the section walk reads, workgroup-uniform
struct VtaFrame {
    const double2* zz;   // LDS: (z_i, 1 / z_i)
    const double* len;   // LDS: l_i
    int n;
    bool equal;          // all n lengths are equal
    double two_pi, c;
    double z_last, a_last;   // rho c / A_K and sqrt(A_K / pi); z_last = 0 without radiation
};

// den(f) = C Z + D of the frame
__device__ __forceinline__ void vta_den(const VtaFrame& fr, double f, double* re, double* im) {
    const double k = fr.two_pi * f / fr.c;
    double c_ = 0.0, d = 1.0, sn = 0.0, cs = 1.0;
    if (fr.equal) sincos(k * fr.len[0], &sn, &cs);
    for (int i = 0; i < fr.n; ++i) {
        if (!fr.equal) sincos(k * fr.len[i], &sn, &cs);
        const double2 z = fr.zz[i];
        const double c2 = c_ * cs + d * (sn * z.y);
        d = d * cs - c_ * (z.x * sn);
        c_ = c2;
    }
    if (fr.z_last != 0.0) {
        const double ka = fr.two_pi * f * fr.a_last / fr.c;
        *re = d - c_ * (fr.z_last * (8.0 * ka / (3.0 * M_PI)));
        *im = c_ * (fr.z_last * (ka * ka / 2.0));
    } else {
        *re = d;
        *im = 0.0;
    }
}

__global__ __launch_bounds__(VTA_THREADS) void vta_kernel(VtaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vta_lds[];
    __shared__ int s_min[VTA_MAX_FORMANTS];
    __shared__ int s_found;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long frame = blockIdx.x;
    const int K = a.K, F = a.F;
    double2* s_zz = reinterpret_cast<double2*>(vta_lds);   // [K]
    double* s_len = reinterpret_cast<double*>(s_zz + K);   // [K]
    double* s_g = s_len + K;                               // [F]

    // 1. staging
    int n = a.counts ? a.counts[frame] : K;
    n = n > K ? K : n;
    const double* pa = a.areas + frame * a.a_frame;
    const double* pl = a.lengths + frame * a.l_frame;
    const double rc = a.rho * a.c;
    const double l0 = n >= 1 ? pl[0] : 0.0;
    int bad = n < 1 ? 1 : 0, closed = 0, unequal = 0;
    for (int i = tid; i < n; i += VTA_THREADS) {
        double A = pa[i * a.a_sec];
        const double l = pl[i * a.l_sec];
        if (!(isfinite(A) && isfinite(l) && l > 0.0)) bad = 1;
        if (A < a.min_area) {
            A = a.min_area;
            closed = 1;
        }
        if (l != l0) unequal = 1;
        s_zz[i] = make_double2(rc / A, A / rc);
        s_len[i] = l;
    }
    bad = __syncthreads_or(bad);   // the votes are the barrier behind the staging
    closed = __syncthreads_or(closed);
    unequal = __syncthreads_or(unequal);
    if (tid == 0 && a.status) a.status[frame] = (closed ? 1 : 0) | (bad ? 2 : 0);
    double2* o_den = a.den ? reinterpret_cast<double2*>(a.den) + frame * F : nullptr;
    double2* o_h = a.transfer ? reinterpret_cast<double2*>(a.transfer) + frame * F : nullptr;
    double* o_freq = a.freq ? a.freq + frame * a.n_formants : nullptr;
    double* o_level = a.level ? a.level + frame * a.n_formants : nullptr;
    if (bad) {   // workgroup-uniform: NaN in every output of this frame, nothing else of it is computed
        for (int j = tid; j < F; j += VTA_THREADS) {
            if (o_den) o_den[j] = make_double2(NAN, NAN);
            if (o_h) o_h[j] = make_double2(NAN, NAN);
        }
        if (tid < a.n_formants) {
            if (o_freq) o_freq[tid] = NAN;
            if (o_level) o_level[tid] = NAN;
        }
        if (tid == 0 && a.found) a.found[frame] = 0;
        return;
    }
    VtaFrame fr;
    fr.zz = s_zz;
    fr.len = s_len;
    fr.n = n;
    fr.equal = !unequal;
    fr.two_pi = 2.0 * M_PI;
    fr.c = a.c;
    fr.z_last = 0.0;
    fr.a_last = 0.0;
    if (a.radiation) {
        double A = pa[(long)(n - 1) * a.a_sec];
        A = A < a.min_area ? a.min_area : A;
        fr.z_last = rc / A;
        fr.a_last = sqrt(A / M_PI);
    }

    // 2. the bins
    for (int j = tid; j < F; j += VTA_THREADS) {
        double re, im;
        vta_den(fr, a.f0 + (double)j * a.df, &re, &im);
        const double g = re * re + im * im;
        s_g[j] = g;
        if (o_den) o_den[j] = make_double2(re, im);
        if (o_h) o_h[j] = make_double2(re / g, -im / g);
    }
    __syncthreads();

    // 3. coarse minima, in order
    if (wave == 0) {
        int cnt = 0;
        for (int j0 = 1; j0 < F - 1 && cnt < a.n_formants; j0 += 64) {   // wave-uniform
            const int j = j0 + lane;
            bool is_min = false;
            if (j < F - 1) {
                const double g = s_g[j];
                is_min = g < s_g[j - 1] && g <= s_g[j + 1];
            }
            const unsigned long long votes = __ballot(is_min);
            const int slot = cnt + __popcll(votes & ((1ull << lane) - 1ull));
            if (is_min && slot < a.n_formants) s_min[slot] = j;
            cnt += __popcll(votes);
        }
        cnt = cnt > a.n_formants ? a.n_formants : cnt;
        if (lane == 0) {
            s_found = cnt;
            if (a.found) a.found[frame] = cnt;
        }
    }
    __syncthreads();

    // 4. refinement: a wave per formant, a lane per probe
    const int nf = s_found;
    for (int s = wave; s < a.n_formants; s += VTA_WAVES) {   // wave-uniform
        double mid = NAN, lvl = NAN;
        if (s < nf) {
            const int j = s_min[s];
            double lo = a.f0 + (double)(j - 1) * a.df, hi = a.f0 + (double)(j + 1) * a.df;
            double at = a.f0 + (double)j * a.df, g_at = s_g[j];   // the bracket's midpoint and g there: bin j before any round
            for (int r = 0; r < a.rounds; ++r) {
                const double w = (hi - lo) / (double)(VTA_PROBES + 1);
                double re, im;
                vta_den(fr, lo + w * (double)(lane + 1), &re, &im);
                double g = re * re + im * im;
                int m = lane + 1;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double og = __shfl_xor(g, o, 64);
                    const int om = __shfl_xor(m, o, 64);
                    if (og < g || (og == g && om < m)) {
                        g = og;
                        m = om;
                    }
                }
                m = __shfl(m, 0, 64);
                g_at = __shfl(g, 0, 64);
                at = lo + w * (double)m;   // the winner's own frequency, bit for bit
                lo = at - w;
                hi = at + w;
            }
            mid = at;
            lvl = -10.0 * log10(g_at);
        }
        if (lane == 0) {
            if (o_freq) o_freq[s] = mid;
            if (o_level) o_level[s] = lvl;
        }
    }
}

}  // namespace

extern "C" int as_vt_acoustics(const double* areas, int64_t a_frame, int64_t a_sec, const double* lengths, int64_t l_frame,
                               int64_t l_sec, const int32_t* counts, int64_t frames, int32_t K, double f0, double df, int32_t F,
                               int32_t radiation, double c, double rho, double min_area, int32_t n_formants, int32_t rounds,
                               double* den, double* transfer, double* freq, double* level, int32_t* found, int32_t* status,
                               void* stream) {
    AS_REQUIRE(areas && lengths && frames >= 0 && frames <= 0x7fffffff, AS_ERR_BAD_ARG, "as_vt_acoustics: bad argument");
    AS_REQUIRE(K >= 1 && K <= VTA_MAX_K, AS_ERR_BAD_ARG, "as_vt_acoustics: %d sections (1 .. %d supported)", K, VTA_MAX_K);
    AS_REQUIRE(F >= 3 && F <= VTA_MAX_F, AS_ERR_BAD_ARG, "as_vt_acoustics: %d frequency bins (3 .. %d supported)", F, VTA_MAX_F);
    AS_REQUIRE(n_formants >= 0 && n_formants <= VTA_MAX_FORMANTS, AS_ERR_BAD_ARG, "as_vt_acoustics: %d formants (0 .. %d supported)",
               n_formants, VTA_MAX_FORMANTS);
    AS_REQUIRE(rounds >= 0 && rounds <= VTA_MAX_ROUNDS, AS_ERR_BAD_ARG, "as_vt_acoustics: %d refinement rounds (0 .. %d supported)",
               rounds, VTA_MAX_ROUNDS);
    AS_REQUIRE(f0 > 0.0 && df > 0.0 && isfinite(f0) && isfinite(df), AS_ERR_BAD_ARG,
               "as_vt_acoustics: the grid f0 + j df needs f0 > 0 and df > 0 (got %g, %g)", f0, df);
    AS_REQUIRE(c > 0.0 && rho > 0.0 && min_area > 0.0 && isfinite(c) && isfinite(rho) && isfinite(min_area), AS_ERR_BAD_ARG,
               "as_vt_acoustics: c, rho and min_area must be positive (got %g, %g, %g)", c, rho, min_area);
    AS_REQUIRE(radiation == 0 || radiation == 1, AS_ERR_BAD_ARG, "as_vt_acoustics: radiation %d (0 = open end, 1 = piston)", radiation);
    AS_REQUIRE(as_aligned16(den) && as_aligned16(transfer), AS_ERR_BAD_ARG,
               "as_vt_acoustics: den and transfer hold complex128 values and must be 16-byte aligned");
    if (frames == 0) return 0;
    VtaArgs a;
    a.areas = areas;
    a.a_frame = (long)a_frame;
    a.a_sec = (long)a_sec;
    a.lengths = lengths;
    a.l_frame = (long)l_frame;
    a.l_sec = (long)l_sec;
    a.counts = counts;
    a.K = K;
    a.F = F;
    a.radiation = radiation;
    a.n_formants = n_formants;
    a.rounds = rounds;
    a.f0 = f0;
    a.df = df;
    a.c = c;
    a.rho = rho;
    a.min_area = min_area;
    a.den = den;
    a.transfer = transfer;
    a.freq = freq;
    a.level = level;
    a.found = found;
    a.status = status;
    const size_t lds = (size_t)(3 * K + F) * sizeof(double);   // <= 56 KiB
    hipLaunchKernelGGL(vta_kernel, dim3((unsigned)frames), dim3(VTA_THREADS), lds, (hipStream_t)stream, a);
    AS_LAUNCH_CHECK("as_vt_acoustics");
    return 0;
}
