// Contour smoothing on the device: a penalised least-squares B-spline through every contour of a batch, in one launch.  The
// reference smooths each predicted contour with vt_tools.bs_regularization.regularize_Bsplines(contour, 3) before it saves it
// (generate_vocal_tract_shape_v2.py:173,252, generate_vocal_tract_shape.py:155, phoneme_to_articulation/__init__.py:178-180).
// vt_tools is neither vendored nor pinned by the reference, so the definition below is THIS PROJECT'S OWN and its
// parity with vt_tools is unpinned -- an ASSUMPTION, like load_articulator_array and the torchaudio restatements.
//
// One contour of N points p_i (float32, widened to float64 once), degree d in {1, 2, 3}, K control points, M outputs:
//   parameter   s_0 = 0, s_i = s_{i-1} + |p_i - p_{i-1}|, u_i = s_i / s_{N-1}, u_{N-1} = 1; s_{N-1} == 0: every output is p_0, copied
//   basis       clamped uniform knots [0]*d + linspace(0, 1, K-d+1) + [1]*d; span(u) = min(floor(u (K-d)), K-d-1); Cox-de Boor
//   fit         (B'B + lambda D'D) c = B'p with D the second difference of the control points; x and y are two right-hand
//               sides of one symmetric positive definite band matrix (half-bandwidth max(d, 2)); square-root-free banded
//               Cholesky, A = L diag(d) L'
//   evaluate    at v_m = m / (M-1), rounded to float32 once
//
// cs_kernel<D>: one wave per contour, four waves (contours) per workgroup, no workgroup barrier -- a wave that has nothing to fit
// (padding, a non-finite point, zero length) leaves early.  Everything a wave shares between its lanes lives in its own slice
// of LDS, sized by N (2000 + 44 N bytes: 4.1 KiB at N = 50, 13 KiB at the limit), ordered by wave-level fences:
//   1. lanes own points: load, non-finite vote, chord lengths, a wave scan (shuffles, fixed order) for s, the basis values and
//      span of every point -> LDS, value-major so that lanes on adjacent points touch adjacent banks; the recursion's
//      denominators are knot differences, 1, 2 or 3 grid steps on the uniform vector, so it multiplies by constants;
//   2. one lane per band entry of B'B (and per entry of B'p) walks the points whose span reaches it, span by span in point order
//      -- spans grow with the point index, so the points of a span are one index range, found by bisection; no atomics of any
//      kind, the order of every sum is fixed and two launches give equal bits;
//   3. lanes 0 and 1 factorise (the columns of L slide through registers; at most 32 columns of 4; one v_rcp_f64 with two Newton
//      steps per column, no square root) and each substitutes one coordinate forwards and backwards;
//   4. lanes own outputs: basis at v_m, <= 4 control points from LDS, one float store.
// float64 throughout: the systems reach condition numbers of 1e7, where a float32 solve is off by 2.5e-3 on unit-square contours.
#include <math.h>

#include "as_common.h"
#include "as_device.h"
#include "as_launch.h"

namespace {

constexpr int CS_WAVES = 4;       // contours per workgroup
constexpr int CS_MAX_N = 256;     // points per contour: four passes of one point per lane
constexpr int CS_MAX_K = 32;
constexpr int CS_MAX_M = 1024;
constexpr int CS_BAND = 4;        // stored band: the diagonal and three above it (max(d, 2) used, the rest zero)
constexpr int CS_KNOTS = CS_MAX_K + 4 + 4;   // K + d + 1 <= 36, padded
constexpr int CS_FIRST = CS_MAX_K + 4;       // K - d + 1 <= 32 range starts, padded

// this wave's LDS writes are visible to its other lanes: LDS operations of one wave complete in order, the fence keeps the
// compiler from moving accesses across
__device__ __forceinline__ void cs_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 1 / d in float64 without the division sequence: v_rcp_f64 (about 2^-23 relative) and two Newton steps
__device__ __forceinline__ double cs_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    return fma(fma(-d, r, 1.0), r, r);
}

// The D + 1 basis functions that are non-zero on span `span` (control points span .. span + D) at u; kt: the knot vector.
// Cox-de Boor's denominators are differences of two knots, on the uniform clamped vector m / nsp with m = 1, 2 or 3 counted on
// the integer grid: their reciprocals are nsp, nsp / 2, nsp / 3 (scale[m]), so no point pays a float64 division.
template <int D>
__device__ __forceinline__ void cs_basis(double u, int span, const double* kt, int nsp, const double (&scale)[4], double (&nb)[D + 1]) {
    const int k = span + D;
    double left[D + 1], right[D + 1];
    nb[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= D; ++j) {
        left[j] = u - kt[k + 1 - j];
        right[j] = kt[k + j] - u;
        double saved = 0.0;
#pragma unroll
        for (int r = 0; r < j; ++r) {
            const int hi = span + r + 1 < nsp ? span + r + 1 : nsp, lo = span + r + 1 - j > 0 ? span + r + 1 - j : 0;
            const int m = hi - lo;   // knots k + r + 1 and k + r + 1 - j: 1 <= m <= j
            const double temp = nb[r] * (m == 1 ? scale[1] : (m == 2 ? scale[2] : scale[3]));
            nb[r] = saved + right[r + 1] * temp;
            saved = left[j - r] * temp;
        }
        nb[j] = saved;
    }
}

__host__ __device__ inline int cs_np(int N) { return (N + 1) & ~1; }
// bytes of LDS of one wave: doubles kt | band | rhs | basis values [4][np], floats px | py [np], ints span [np] | first
__host__ __device__ inline int cs_wave_bytes(int N) {
    const int np = cs_np(N);
    const int b = 8 * (CS_KNOTS + CS_MAX_K * CS_BAND + 2 * CS_MAX_K + 4 * np) + 4 * (2 * np) + 4 * (np + CS_FIRST);
    return (b + 15) & ~15;
}

template <int D>
__global__ __launch_bounds__(CS_WAVES * 64) void cs_kernel(const float* __restrict__ in, long s_contour, long s_coord, long s_point,
                                                           long n_contours, int N, int K, double lambda, int M,
                                                           const int64_t* __restrict__ lengths, int T, int A,
                                                           float* __restrict__ out, long out_pitch, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * CS_WAVES + wave;
    if (c >= n_contours) return;   // wave-uniform, and no workgroup barrier anywhere below
    float* ox = out + c * 2 * out_pitch;
    float* oy = ox + out_pitch;
    if (lengths) {
        const long per = (long)T * A;
        const long b = c / per, t = (c % per) / A;
        if (t >= lengths[b]) {   // a padded frame: zeros, like padded positions elsewhere
            for (int m = lane; m < M; m += 64) ox[m] = oy[m] = 0.f;
            if (status && lane == 0) status[c] = 0;
            return;
        }
    }
    const int np = cs_np(N), nsp = K - D;
    const double scale[4] = {0.0, (double)nsp, (double)nsp * 0.5, (double)nsp * (1.0 / 3.0)};   // nsp / (knots apart)
    unsigned char* base = cs_lds + (size_t)wave * cs_wave_bytes(N);
    double* kt = reinterpret_cast<double*>(base);
    double* band = kt + CS_KNOTS;              // [K][CS_BAND]: A(j, j + r), then L(j + r, j)
    double* rhs = band + CS_MAX_K * CS_BAND;   // [2][CS_MAX_K]: B'p, then the control points
    double* bv = rhs + 2 * CS_MAX_K;           // [4][np] basis values of the points
    float* px = reinterpret_cast<float*>(bv + 4 * np);
    float* py = px + np;
    int* sp = reinterpret_cast<int*>(py + np);
    int* first = sp + np;                      // first[k] = the first point whose span is >= k; first[nsp] = N

    // 1. points
    const float* pc = in + c * s_contour;
    bool finite = true;
    for (int i = lane; i < N; i += 64) {
        const float x = pc[i * s_point], y = pc[s_coord + i * s_point];
        finite = finite && isfinite(x) && isfinite(y);
        px[i] = x;
        py[i] = y;
    }
    for (int j = lane; j < K + D + 1; j += 64) {
        const int q = j - D;
        kt[j] = q <= 0 ? 0.0 : (q >= nsp ? 1.0 : (double)q / (double)nsp);
    }
    if (__ballot(!finite) != 0ull) {   // a non-finite coordinate: NaN in this row only
        for (int m = lane; m < M; m += 64) ox[m] = oy[m] = NAN;
        if (status && lane == 0) status[c] = 2;
        return;
    }
    cs_wave_sync();
    double s[CS_MAX_N / 64];
    double carry = 0.0;
#pragma unroll
    for (int q = 0; q < CS_MAX_N / 64; ++q) {
        s[q] = 0.0;
        if (q * 64 < N) {   // wave-uniform
            const int i = q * 64 + lane;
            double seg = 0.0;
            if (i >= 1 && i < N) {
                const double dx = (double)px[i] - (double)px[i - 1], dy = (double)py[i] - (double)py[i - 1];
                seg = sqrt(dx * dx + dy * dy);
            }
            s[q] = carry + as_wave_scan(seg, lane, AsAdd{});
            carry = __shfl(s[q], 63, 64);
        }
    }
    const double total = carry;   // s_{N-1}: the points past N add zero
    if (!(total > 0.0)) {         // zero length: p_0, copied
        const float x0 = px[0], y0 = py[0];
        for (int m = lane; m < M; m += 64) {
            ox[m] = x0;
            oy[m] = y0;
        }
        if (status && lane == 0) status[c] = 1;
        return;
    }
#pragma unroll
    for (int q = 0; q < CS_MAX_N / 64; ++q) {
        const int i = q * 64 + lane;
        if (i < N) {
            const double u = i == N - 1 ? 1.0 : s[q] / total;
            int span = (int)(u * (double)nsp);
            span = span > nsp - 1 ? nsp - 1 : span;
            double nb[D + 1];
            cs_basis<D>(u, span, kt, nsp, scale, nb);
#pragma unroll
            for (int t = 0; t <= D; ++t) bv[t * np + i] = nb[t];
            sp[i] = span;
        }
    }
    cs_wave_sync();
    if (lane <= nsp) {   // nsp <= 31
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sp[mid] < lane) lo = mid + 1;
            else hi = mid;
        }
        first[lane] = lo;
    }
    cs_wave_sync();

    // 2. normal equations: K * CS_BAND band entries, then 2 K right-hand sides, one lane each
    for (int e = lane; e < K * CS_BAND + 2 * K; e += 64) {
        double acc = 0.0;
        if (e < K * CS_BAND) {
            const int j = e / CS_BAND, r = e % CS_BAND, col = j + r;
            if (col < K && r <= D) {
                const int klo = col - D > 0 ? col - D : 0, khi = j < nsp - 1 ? j : nsp - 1;
                for (int s = klo; s <= khi; ++s) {   // the points of span s in point order: function j is its (j - s)-th
                    const double* ba = bv + (j - s) * np;
                    const double* bb = ba + r * np;
                    const int i1 = first[s + 1];
                    for (int i = first[s]; i < i1; ++i) acc += ba[i] * bb[i];
                }
            }
            if (col < K && r <= 2) {   // lambda D'D, D [K-2][K] = rows (1, -2, 1)
                const int m0 = col - 2 > 0 ? col - 2 : 0, m1 = j < K - 3 ? j : K - 3;
                double pen = 0.0;
                for (int m = m0; m <= m1; ++m) {
                    const int a = j - m, b = col - m;
                    pen += (a == 1 ? -2.0 : 1.0) * (b == 1 ? -2.0 : 1.0);
                }
                acc += lambda * pen;
            }
            band[e] = acc;
        } else {
            const int e2 = e - K * CS_BAND, xy = e2 / K, j = e2 % K;
            const float* p = xy ? py : px;
            const int klo = j - D > 0 ? j - D : 0, khi = j < nsp - 1 ? j : nsp - 1;
            for (int s = klo; s <= khi; ++s) {
                const double* ba = bv + (j - s) * np;
                const int i1 = first[s + 1];
                for (int i = first[s]; i < i1; ++i) acc += ba[i] * (double)p[i];
            }
            rhs[xy * CS_MAX_K + j] = acc;
        }
    }
    cs_wave_sync();

    // 3. A = L diag(d) L' (the square-root-free Cholesky: d_j > 0), the last three columns of L in registers; both lanes
    //    factorise, lane 0 substitutes x and lane 1 y: L z = b, y = z / d, then L' c = y
    if (lane < 2) {
        double* b = rhs + lane * CS_MAX_K;
        double l1[CS_BAND] = {0, 0, 0, 0}, l2[CS_BAND] = {0, 0, 0, 0}, l3[CS_BAND] = {0, 0, 0, 0};   // columns j-1, j-2, j-3
        double d1 = 0.0, d2 = 0.0, d3 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
        for (int j = 0; j < K; ++j) {
            double a[CS_BAND];
#pragma unroll
            for (int r = 0; r < CS_BAND; ++r) a[r] = band[j * CS_BAND + r];
            // A(j + r, j) - sum_m L(j + r, j - m) d_{j-m} L(j, j - m), L(j + r, j - m) = column (j - m)[r + m]
            const double v1 = l1[1] * d1, v2 = l2[2] * d2, v3 = l3[3] * d3;
            const double d = a[0] - (l1[1] * v1 + l2[2] * v2 + l3[3] * v3), inv = cs_rcp(d);
            a[1] -= l1[2] * v1 + l2[3] * v2;
            a[2] -= l1[3] * v1;
            const double z = b[j] - (l1[1] * z1 + l2[2] * z2 + l3[3] * z3);
#pragma unroll
            for (int r = 0; r < CS_BAND; ++r) {
                l3[r] = l2[r];
                l2[r] = l1[r];
            }
            l1[1] = a[1] * inv;
            l1[2] = a[2] * inv;
            l1[3] = a[3] * inv;
            d3 = d2;
            d2 = d1;
            d1 = d;
            z3 = z2;
            z2 = z1;
            z1 = z;
            b[j] = z * inv;
            if (lane == 0) {
                band[j * CS_BAND + 1] = l1[1];
                band[j * CS_BAND + 2] = l1[2];
                band[j * CS_BAND + 3] = l1[3];
            }
        }
    }
    cs_wave_sync();
    if (lane < 2) {
        double* b = rhs + lane * CS_MAX_K;
        double c1 = 0.0, c2 = 0.0, c3 = 0.0;   // c_{j+1}, c_{j+2}, c_{j+3}
        for (int j = K - 1; j >= 0; --j) {
            const double v = b[j] - (band[j * CS_BAND + 1] * c1 + band[j * CS_BAND + 2] * c2 + band[j * CS_BAND + 3] * c3);
            c3 = c2;
            c2 = c1;
            c1 = v;
            b[j] = v;
        }
    }
    cs_wave_sync();

    // 4. evaluation
    const double inv_m = 1.0 / (double)(M - 1);
    for (int m = lane; m < M; m += 64) {
        const double v = m == M - 1 ? 1.0 : (double)m * inv_m;
        int span = (int)(v * (double)nsp);
        span = span > nsp - 1 ? nsp - 1 : span;
        double nb[D + 1];
        cs_basis<D>(v, span, kt, nsp, scale, nb);
        double x = 0.0, y = 0.0;
#pragma unroll
        for (int t = 0; t <= D; ++t) {
            x += nb[t] * rhs[span + t];
            y += nb[t] * rhs[CS_MAX_K + span + t];
        }
        ox[m] = (float)x;
        oy[m] = (float)y;
    }
    if (status && lane == 0) status[c] = 0;
}

}  // namespace

extern "C" int as_contour_spline(const float* contours, int64_t s_contour, int64_t s_coord, int64_t s_point, int64_t n_contours,
                                 int32_t N, int32_t K, int32_t degree, double lambda, int32_t M, const int64_t* lengths, int32_t T,
                                 int32_t A, float* out, int64_t out_pitch, int32_t* status, void* stream) {
    AS_REQUIRE(contours && out && n_contours >= 0 && out_pitch >= M, AS_ERR_BAD_ARG, "as_contour_spline: bad argument");
    AS_REQUIRE(degree >= 1 && degree <= 3, AS_ERR_UNSUPPORTED, "as_contour_spline: degree %d (1, 2 or 3 supported)", degree);
    AS_REQUIRE(N >= 2 && N <= CS_MAX_N, AS_ERR_UNSUPPORTED, "as_contour_spline: %d points per contour (2 .. %d supported)", N, CS_MAX_N);
    AS_REQUIRE(K >= degree + 1 && K <= CS_MAX_K, AS_ERR_UNSUPPORTED, "as_contour_spline: %d control points (%d .. %d supported)", K,
               degree + 1, CS_MAX_K);
    AS_REQUIRE(M >= 2 && M <= CS_MAX_M, AS_ERR_UNSUPPORTED, "as_contour_spline: %d output points (2 .. %d supported)", M, CS_MAX_M);
    AS_REQUIRE(lambda > 0.0 && isfinite(lambda), AS_ERR_BAD_ARG,
               "as_contour_spline: lambda must be positive and finite (0 leaves clustered points a singular matrix)");
    AS_REQUIRE(!lengths || (T > 0 && A > 0 && n_contours % ((int64_t)T * A) == 0), AS_ERR_BAD_ARG,
               "as_contour_spline: lengths need n_contours = B * T * A");
    AS_REQUIRE(n_contours <= (int64_t)0x7fffffff * CS_WAVES, AS_ERR_UNSUPPORTED, "as_contour_spline: too many contours");
    if (n_contours == 0) return 0;
    const unsigned grid = (unsigned)((n_contours + CS_WAVES - 1) / CS_WAVES);
    const size_t lds = (size_t)CS_WAVES * cs_wave_bytes(N);   // <= 54 KiB
    int rc = 0;
    as_exactly<1, 2, 3>(degree, &rc, [&](auto d) {
        hipLaunchKernelGGL(cs_kernel<decltype(d)::value>, dim3(grid), dim3(CS_WAVES * 64), lds, (hipStream_t)stream, contours,
                           (long)s_contour, (long)s_coord, (long)s_point, (long)n_contours, N, K, lambda, M, lengths, T, A, out,
                           (long)out_pitch, status);
        return 0;
    });
    AS_LAUNCH_CHECK("as_contour_spline");
    return rc;
}
