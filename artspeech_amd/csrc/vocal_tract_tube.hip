// The vocal-tract tube on the device: the internal and the external wall of every frame of a batch, from the frame's articulator
// contours, in one launch.  The reference obtains the two walls from vt_shape_gen.vocal_tract_tube.generate_vocal_tract_tube
// (generate_vocal_tract_shape_v2.py:426, generate_vocal_tract_shape.py:34, scripts/shape_to_air_column.py:77).  vt_shape_gen is
// neither vendored nor pinned by the reference, so the definition below is THIS PROJECT'S OWN and its parity with
// vt_shape_gen is unpinned -- an ASSUMPTION, like load_articulator_array and regularize_Bsplines.
//
// A wall is built from a chain of K contours c_0 .. c_{K-1} (1 <= K <= 8), each an open polyline of N float32 points.  Nothing
// below depends on the orientation in which a contour's points are stored.
//   junctions   for k < K-1, (i_k, j_k) minimises |c_k[i] - c_{k+1}[j]|^2 over the N x N pairs; the squared distance is float32,
//               dx*dx + dy*dy of direct differences, multiply and add not contracted (as_p2cp_scan_argmin's expression); among
//               equal minima the lowest i, then the lowest j (the first minimum in row-major order); junctions are independent
//   runs        contour k contributes its points from entry e_k to exit x_k inclusive, ascending if e_k <= x_k, else descending.
//               interior: e_k = j_{k-1}, x_k = i_k.  first: e_0 = 0 if i_0 >= N-1-i_0, else N-1 (the end with more points before the
//               exit, a tie gives 0).  last: x_{K-1} = N-1 if e_{K-1} <= N-1-e_{K-1}, else 0.  K = 1: 0 .. N-1.
//               The wall's polyline is the concatenation of the runs: P points, K <= P <= K N; the jump from c_k[x_k] to
//               c_{k+1}[e_{k+1}] is one of its segments and may have length zero.
//   resampling  float64: the points widened exactly, s_0 = 0, s_p = s_{p-1} + sqrt(dx^2 + dy^2), L = s_{P-1}; output m of M sits at
//               t = (m L) / (M-1): p the largest index with s_p <= t, clipped to P-2, f = (t - s_p) / (s_{p+1} - s_p) (0 on a
//               segment of zero length), q_p + f (q_{p+1} - q_p).  Output 0 is the first and output M-1 the last point, copied.
//   status      bit 0: L == 0, every output is the first point.  bit 1: a NaN or infinite coordinate in a chain contour, every
//               output is NaN and the wall's junctions are -1.
//
// vtt_kernel: one wave per (frame, wall), four waves per workgroup, no workgroup barrier -- a wave whose frame lies behind its
// sentence's length, or that saw a non-finite point, leaves early.  A wave's slice of LDS holds its chain's contours (float32,
// x | y per contour, each padded to a multiple of 4 points with +inf as the closest-point scan wants) and the arc lengths s:
// 16 K ceil4(N) bytes, 4.9 KiB with the defaults, 16 KiB at the limits (64 KiB a workgroup: no grant needed).  The run points
// themselves are not copied: point p of the polyline is point e_k +- (p - first_k) of contour k, read from the contour where
// it lies and widened there; the table of runs is held by the lanes (lane k: contour k) and read with a shuffle.
//   1. junction search: lanes own the points i of c_k in passes of 64, each scans c_{k+1} in LDS (as_p2cp_scan_argmin: the lowest
//      j of the lane's minimum), then a wave arg-min over (value, i) with the lowest i;
//   2. arc length: lanes own the polyline's points in passes of 64, a wave scan (shuffles, fixed order) with a carry gives s;
//   3. outputs: lanes own the outputs m, each bisects s in LDS, then one lerp and two float64 stores.
// No atomics, every sum in a fixed order: two launches give equal bits, and a frame alone or inside a batch gives equal bits.
// The file is built with -ffp-contract=off: the junction indices equal those of an op-by-op float32 restatement, and the lerp is
// numpy's expression.
#include <math.h>

#include "as_common.h"
#include "as_device.h"

namespace {

constexpr int VTT_WAVES = 4;     // (frame, wall) pairs per workgroup
constexpr int VTT_MAX_N = 128;   // points per contour: two passes of one point per lane
constexpr int VTT_MAX_K = 8;     // contours per chain
constexpr int VTT_MAX_M = 1024;

struct VttChains { int art[2][VTT_MAX_K]; };   // by value in the kernel arguments: 64 bytes, checked on the host

__device__ __forceinline__ void vtt_wave_sync() {   // this wave's LDS writes are visible to its other lanes (cs_wave_sync)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__host__ __device__ inline int vtt_np(int N) { return (N + 3) & ~3; }
// bytes of LDS of one wave: floats [K][2][np] contours, doubles s [K * np]; a multiple of 16
__host__ __device__ inline int vtt_wave_bytes(int N, int K) { return 16 * K * vtt_np(N); }

// The runs of a wall live in the lanes, not in memory: lane k holds contour k's run as one word, the polyline index of its first
// point (< 1024: bits 0-10), its entry index (< 128: bits 11-17) and bit 18 where it descends.  first[q], q = 1 .. 7, are also
// kept as wave-uniform values (v_readlane) to find the contour of a point; lanes at or past K hold first = P, above every point.
struct VttRuns {
    int word;                  // this lane's run
    int first[VTT_MAX_K];      // wave-uniform, [0] unused
};

// point p of the polyline, widened to float64: seven comparisons, one lane-indexed shuffle, two LDS reads
__device__ __forceinline__ void vtt_point(const VttRuns& r, const float* cont, int np, int p, double* x, double* y) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < VTT_MAX_K; ++q) k += p >= r.first[q] ? 1 : 0;
    const int word = __shfl(r.word, k, 64);
    const int d = p - (word & 0x7ff), e = (word >> 11) & 0x7f;
    const int i = (word >> 18) ? e - d : e + d;
    const float* c = cont + (size_t)k * 2 * np;
    *x = (double)c[i];
    *y = (double)c[np + i];
}

__global__ __launch_bounds__(VTT_WAVES * 64) void vtt_kernel(const float* __restrict__ in, long s_frame, long s_art, long s_coord,
                                                             long s_point, long frames, int N, VttChains chains, int k_int,
                                                             int k_ext, const int64_t* __restrict__ lengths, int T, int M,
                                                             double* __restrict__ air, long ld_out, int* __restrict__ status,
                                                             int* __restrict__ junctions, double* __restrict__ wall_length) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vtt_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * VTT_WAVES + wave;   // frame * 2 + wall
    if (w >= frames * 2) return;   // wave-uniform, and no workgroup barrier anywhere below
    const long frame = w >> 1;
    const int wall = (int)(w & 1);
    const int K = wall ? k_ext : k_int, k_lds = k_int > k_ext ? k_int : k_ext;
    double* ox = air + w * 2 * ld_out;
    double* oy = ox + ld_out;
    int* jn = junctions ? junctions + w * 2 * (VTT_MAX_K - 1) : nullptr;
    if (lengths) {
        const long b = frame / T, t = frame % T;
        if (t >= lengths[b]) {   // a padded frame: zeros, like padded positions elsewhere; its contours are not read
            for (int m = lane; m < M; m += 64) ox[m] = oy[m] = 0.0;
            if (jn && lane < 2 * (VTT_MAX_K - 1)) jn[lane] = -1;
            if (lane == 0) {
                if (status) status[w] = 0;
                if (wall_length) wall_length[w] = 0.0;
            }
            return;
        }
    }
    const int np = vtt_np(N);
    unsigned char* base = vtt_lds + (size_t)wave * vtt_wave_bytes(N, k_lds);
    float* cont = reinterpret_cast<float*>(base);                           // [K][2][np]
    double* s = reinterpret_cast<double*>(base + (size_t)8 * k_lds * np);   // [<= K N]

    // the chain's contours, padded with +inf
    bool finite = true;
#pragma unroll
    for (int k = 0; k < VTT_MAX_K; ++k) {
        if (k < K) {   // wave-uniform
            const int a = wall ? chains.art[1][k] : chains.art[0][k];
            const float* pc = in + frame * s_frame + (long)a * s_art;
            float* cx = cont + (size_t)k * 2 * np;
            for (int i = lane; i < np; i += 64) {
                float x = INFINITY, y = INFINITY;
                if (i < N) {
                    x = pc[i * s_point];
                    y = pc[s_coord + i * s_point];
                    finite = finite && isfinite(x) && isfinite(y);
                }
                cx[i] = x;
                cx[np + i] = y;
            }
        }
    }
    if (__ballot(!finite) != 0ull) {   // a non-finite coordinate: NaN in this wall only, junctions -1
        for (int m = lane; m < M; m += 64) ox[m] = oy[m] = NAN;
        if (jn && lane < 2 * (VTT_MAX_K - 1)) jn[lane] = -1;
        if (lane == 0) {
            if (status) status[w] = 2;
            if (wall_length) wall_length[w] = NAN;
        }
        return;
    }
    vtt_wave_sync();

    // 1. junctions: lane k keeps (i_k, j_k), the point on c_k and the point on c_{k+1}
    int my_i = 0, my_j = 0;
    for (int k = 0; k + 1 < K; ++k) {
        const float* cx = cont + (size_t)k * 2 * np;
        const float* qx = cx + 2 * np;   // c_{k+1}
        float best = INFINITY;
        int bi = 0x7fffffff, bj = 0;
        for (int i0 = 0; i0 < N; i0 += 64) {   // ascending i: a strict < keeps the lane's lowest i
            const int i = i0 + lane;
            if (i < N) {
                float m;
                const int j = as_p2cp_scan_argmin(cx[i], cx[np + i], qx, qx + np, np, &m);
                if (m < best || bi == 0x7fffffff) {
                    best = m;
                    bi = i;
                    bj = j;
                }
            }
        }
        const float vmin = as_wave_min(best);   // lanes without a point hold +inf and an i past every real one
        int cand = best == vmin ? bi : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(cand, o, 64);
            cand = other < cand ? other : cand;
        }
        const int wj = __shfl(bj, cand & 63, 64);   // cand is the best of lane cand & 63: that lane's j goes with it
        if (lane == k) {
            my_i = cand;
            my_j = wj;
        }
    }
    if (jn) {   // all lanes shuffle, fourteen store
        const int q = (lane >> 1) & 7;
        const int vi = __shfl(my_i, q, 64), vj = __shfl(my_j, q, 64);
        if (lane < 2 * (VTT_MAX_K - 1)) jn[lane] = q < K - 1 ? ((lane & 1) ? vj : vi) : -1;
    }

    // 2. runs (lane k: contour k) and arc length
    VttRuns r;
    int P;
    {
        const int prev_j = __shfl_up(my_j, 1, 64);   // j_{k-1} in lane k
        int e = 0, x = N - 1, len = 0;
        if (lane < K) {
            if (K > 1) {
                if (lane == 0) {
                    x = my_i;
                    e = x >= N - 1 - x ? 0 : N - 1;
                } else {
                    e = prev_j;
                    x = lane == K - 1 ? (e <= N - 1 - e ? N - 1 : 0) : my_i;
                }
            }
            len = (e <= x ? x - e : e - x) + 1;
        }
        const int incl = as_wave_scan(len, lane, AsAdd{});
        const int first = incl - len;
        P = __shfl(incl, 63, 64);
        r.word = (first & 0x7ff) | (e << 11) | (e <= x ? 0 : 1 << 18);   // first == P == 1024 only in lanes past K: not read
        r.first[0] = 0;
#pragma unroll
        for (int q = 1; q < VTT_MAX_K; ++q) r.first[q] = __builtin_amdgcn_readlane(first, q);
    }
    double carry = 0.0;
    for (int p0 = 0; p0 < P; p0 += 64) {   // wave-uniform: every lane takes part in the shuffles
        const int p = p0 + lane;
        const bool on = p >= 1 && p < P;
        double x0, y0, x1, y1;
        vtt_point(r, cont, np, on ? p - 1 : 0, &x0, &y0);
        vtt_point(r, cont, np, on ? p : 0, &x1, &y1);
        const double dx = x1 - x0, dy = y1 - y0;
        const double seg = on ? sqrt(dx * dx + dy * dy) : 0.0;
        const double sp = carry + as_wave_scan(seg, lane, AsAdd{});
        if (p < P) s[p] = sp;
        carry = __shfl(sp, 63, 64);   // the points past P add zero
    }
    const double L = carry;
    double fx, fy, lx, ly;
    vtt_point(r, cont, np, 0, &fx, &fy);
    vtt_point(r, cont, np, P - 1, &lx, &ly);
    if (lane == 0 && wall_length) wall_length[w] = L;
    if (!(L > 0.0)) {   // zero length: the first point, copied
        for (int m = lane; m < M; m += 64) {
            ox[m] = fx;
            oy[m] = fy;
        }
        if (status && lane == 0) status[w] = 1;
        return;
    }
    vtt_wave_sync();

    // 3. outputs
    const double dm = (double)(M - 1);
    for (int m0 = 0; m0 < M; m0 += 64) {   // wave-uniform, as above
        const int m = m0 + lane;
        const double t = ((double)m * L) / dm;
        int lo = 0, hi = P - 1;   // s[lo] <= t (s_0 = 0), hi stands for an s above t: the result lies in 0 .. P-2
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s[mid] <= t) lo = mid;
            else hi = mid;
        }
        const double s0 = s[lo], den = s[lo + 1] - s0;
        const double f = den > 0.0 ? (t - s0) / den : 0.0;
        double x0, y0, x1, y1;
        vtt_point(r, cont, np, lo, &x0, &y0);
        vtt_point(r, cont, np, lo + 1, &x1, &y1);
        double x = x0 + f * (x1 - x0), y = y0 + f * (y1 - y0);
        if (m == 0) {
            x = fx;
            y = fy;
        }
        if (m >= M - 1) {
            x = lx;
            y = ly;
        }
        if (m < M) {
            ox[m] = x;
            oy[m] = y;
        }
    }
    if (status && lane == 0) status[w] = 0;
}

}  // namespace

extern "C" int as_vocal_tract_tube(const float* contours, int64_t s_frame, int64_t s_art, int64_t s_coord, int64_t s_point,
                                   int64_t frames, int32_t A, int32_t N, const int32_t* chains, int32_t k_int, int32_t k_ext,
                                   const int64_t* lengths, int32_t T, int32_t M, double* air, int64_t ld_out, int32_t* status,
                                   int32_t* junctions, double* wall_length, void* stream) {
    AS_REQUIRE(contours && chains && air && frames >= 0 && A >= 1, AS_ERR_BAD_ARG, "as_vocal_tract_tube: bad argument");
    AS_REQUIRE(N >= 2 && N <= VTT_MAX_N, AS_ERR_BAD_ARG, "as_vocal_tract_tube: %d points per contour (2 .. %d supported)", N, VTT_MAX_N);
    AS_REQUIRE(k_int >= 1 && k_int <= VTT_MAX_K && k_ext >= 1 && k_ext <= VTT_MAX_K, AS_ERR_BAD_ARG,
               "as_vocal_tract_tube: chains of %d and %d contours (1 .. %d supported)", k_int, k_ext, VTT_MAX_K);
    AS_REQUIRE(M >= 2 && M <= VTT_MAX_M, AS_ERR_BAD_ARG, "as_vocal_tract_tube: %d output points (2 .. %d supported)", M, VTT_MAX_M);
    AS_REQUIRE(ld_out >= M, AS_ERR_BAD_ARG, "as_vocal_tract_tube: output rows of %lld hold no %d points", (long long)ld_out, M);
    VttChains ch;
    for (int wl = 0; wl < 2; ++wl)
        for (int k = 0; k < VTT_MAX_K; ++k) {
            const int a = chains[wl * VTT_MAX_K + k];
            const bool used = k < (wl ? k_ext : k_int);
            AS_REQUIRE(!used || (a >= 0 && a < A), AS_ERR_BAD_ARG,
                       "as_vocal_tract_tube: articulator %d at position %d of the %s chain (0 .. %d)", a, k,
                       wl ? "external" : "internal", A - 1);
            ch.art[wl][k] = used ? a : 0;
        }
    AS_REQUIRE(!lengths || (T > 0 && frames % T == 0), AS_ERR_BAD_ARG, "as_vocal_tract_tube: lengths need frames = B * T");
    AS_REQUIRE(frames <= (int64_t)0x3fffffff * VTT_WAVES, AS_ERR_BAD_ARG, "as_vocal_tract_tube: too many frames");
    if (frames == 0) return 0;
    const unsigned grid = (unsigned)((frames * 2 + VTT_WAVES - 1) / VTT_WAVES);
    const size_t lds = (size_t)VTT_WAVES * vtt_wave_bytes(N, k_int > k_ext ? k_int : k_ext);   // <= 64 KiB
    hipLaunchKernelGGL(vtt_kernel, dim3(grid), dim3(VTT_WAVES * 64), lds, (hipStream_t)stream, contours, (long)s_frame, (long)s_art,
                       (long)s_coord, (long)s_point, (long)frames, N, ch, k_int, k_ext, lengths, T, M, air, (long)ld_out, status,
                       junctions, wall_length);
    AS_LAUNCH_CHECK("as_vocal_tract_tube");
    return 0;
}
