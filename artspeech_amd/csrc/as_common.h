// Shared helpers for the gfx950 kernels of libartspeech_hip.so.
#pragma once
#ifndef AS_HOST_ONLY   // gemm_plan.cpp defines it: plain C++, no HIP header -- the integer helpers below and nothing else
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <stdio.h>

#include "artspeech_hip.h"

#define AS_WAVE 64

void as_set_error(const char* fmt, ...);

#define AS_REQUIRE(cond, code, ...)            \
    do {                                       \
        if (!(cond)) {                         \
            as_set_error(__VA_ARGS__);         \
            return (code);                     \
        }                                      \
    } while (0)

// launch check: kernels are enqueued, never synchronised
#define AS_LAUNCH_CHECK(name)                                                  \
    do {                                                                       \
        hipError_t e__ = hipGetLastError();                                    \
        if (e__ != hipSuccess) {                                               \
            as_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return (int)e__;                                                   \
        }                                                                      \
    } while (0)

#define AS_TRY(expr)            \
    do {                        \
        int r__ = (expr);       \
        if (r__ != 0) return r__; \
    } while (0)

static inline int64_t as_round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static inline int as_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline bool as_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// an integer as a type: hands a compile-time constant to a generic lambda (decltype(arg)::value)
template <int N> struct IC { static constexpr int value = N; };

// A run-time number as a template argument: each helper calls the generic lambda f with the IC<N> it picked, once, and f
// launches the kernel instantiated for decltype(arg)::value.  A dispatch must not instantiate a kernel that is never
// launched: f is instantiated for every N of a list, so a choice with three outcomes is ONE list of three, not two nested flags.
// (The lists are walked by recursion, not by a fold expression: hipcc emitted the kernels of a folded list in reverse order, and
// the code objects are compared with those of the ladders these helpers replaced.)
// First fit over an ascending list: f(IC<N>) for the first N >= v, for the last N otherwise (the caller has checked the
// range); f's result, void included
template <int N, int... Rest, typename F>
auto as_up_to(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) return f(IC<N>{});
    else if (v <= N) return f(IC<N>{});
    else return as_up_to<Rest...>(v, f);
}
// Exact match: v in the list: *rc = f(IC<v>), true; otherwise f is not called, false
template <int N, int... Rest, typename F>
auto as_exactly(int v, int* rc, F&& f) {
    if (v == N) return *rc = f(IC<N>{}), true;
    if constexpr (sizeof...(Rest) > 0) return as_exactly<Rest...>(v, rc, f);
    else return false;
}
// A flag: f(IC<1>) or f(IC<0>); f's result
template <typename F>
auto as_flag(bool on, F&& f) {
    if (on) return f(IC<1>{});
    return f(IC<0>{});
}

// grid of a grid-stride element-wise kernel with 256 threads: a workgroup per 256 elements, at least one, at most 2048
static inline int as_ew_grid(long n) {
    const long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

#ifndef AS_HOST_ONLY
// optional per-phase timing (prof.hip); a no-op unless as_profile_enable(1)
struct AsProfScope {
    AsProfScope(const char* name, hipStream_t st);
    ~AsProfScope();
    const char* name_; hipStream_t st_; void* a_; void* b_;
};
bool as_profile_active();   // as_profile_enable(1) is in force
#define AS_PROF_CAT2(a, b) a##b
#define AS_PROF_CAT(a, b) AS_PROF_CAT2(a, b)
#define AS_PROF(name, st) AsProfScope AS_PROF_CAT(as_prof_scope_, __LINE__)(name, st)
// one named, timed launch sequence
#define AS_STEP(name, st, expr) \
    do {                        \
        AS_PROF(name, st);      \
        AS_TRY(expr);           \
    } while (0)

__device__ __forceinline__ float as_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float as_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float as_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double as_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double as_wave_min_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double as_wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
// Inclusive scan over the 64 lanes: lane l gets op(v_0, ..., v_l), combined in log steps over __shfl_up (lane = threadIdx.x & 63)
struct AsAdd { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct AsMin { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return min(a, b); } };
struct AsMax { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return max(a, b); } };
template <typename T, typename Op>
__device__ __forceinline__ T as_wave_scan(T v, int lane, Op op) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v = op(v, t);
    }
    return v;
}
// A length as the kernels that clamp read it: n into [0, T], in n's own type.  (The CTC kernels refuse instead: ctc_sizes.)
template <typename I>
__device__ __forceinline__ I as_clamp_length(I n, int T) { return n < 0 ? 0 : (n > T ? (I)T : n); }
// ReLU that keeps a NaN a NaN, like torch.relu (fmaxf(NaN, 0) = 0 would hide an invalid activation: the transformer's test
// loop finds utterances with NaN predictions by exactly that propagation, transformer/evaluation.py:69-86)
__device__ __forceinline__ float as_relu(float v) { return v < 0.f ? 0.f : v; }
// v_exp_f32 + v_rcp_f32 (1 ulp each): |abs err| ~ 1e-7, far inside the 1e-4 parity budget, and 3x fewer
// instructions than an IEEE division on the recurrence's critical path
__device__ __forceinline__ float as_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// tanh via one exp; no overflow (exp(+inf) -> inf -> rcp = 0 -> 1)
// (exp(2x) as ONE multiply by 2 log2(e) in front of v_exp_f32)
__device__ __forceinline__ float as_tanh(float x) {
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * 2.8853900817779268f));
}
#endif  // AS_HOST_ONLY
