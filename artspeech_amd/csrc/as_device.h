// Device primitives shared by the gfx950 kernels: vector types, LDS-DMA, wave-uniform global pointers, LDS waits, DPP
// reductions, GELU.  Everything is force-inlined: no symbols.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---- LDS-DMA
__device__ __forceinline__ unsigned as_lds_addr(const float* p) {  // byte address inside the workgroup's LDS, wave-uniform
    return __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(const __attribute__((address_space(3))) float*)p);
}
// One LDS-DMA wave-instruction: 64 lanes x 16 B from per-lane global addresses to 1 KiB of LDS at the wave-uniform byte
// address `lds_dst` (+ lane * 16) (global_load_lds_dwordx4: no VGPR destination, counted by vmcnt).  Inline asm on purpose:
// with the builtin hipcc knows that the instruction writes LDS and puts an s_waitcnt vmcnt(0) in front of the next ds_read --
// every k-tile then waits for the DMAs it has just issued, which drains the ring (seen in the ISA of lin_f32.hip's kernels and
// of a 16-deep k-tile version of wgrad_f32.hip; the rings' counted waits + barriers are what orders a slot's reads behind its
// DMAs).  M0 is compiler-reserved: saved and restored inside the one statement that uses it.
__device__ __forceinline__ void as_glds16(const float* src, unsigned lds_dst) {
    unsigned keep;
    lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);  // derived from the wave index: uniform, but only the hardware knows
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds_dst)
                 : "memory");
}

// ---- global pointers
// a pointer the compiler must treat as wave-uniform (SGPR pair): base of the scalar-base form of a global load, whose lane
// part is then a 32-bit byte offset.  (Without it hipcc re-associates base + lane offset into a loop-invariant 64-bit VECTOR
// address and adds the uniform per-step part to that: two address registers and a 64-bit vector add per load.)
typedef const __attribute__((address_space(1))) char* gptr;   // global address space (the integer round trip would lose it: flat loads)
typedef const __attribute__((address_space(1))) f32x4* gptr_f4;
typedef const __attribute__((address_space(1))) u32x4* gptr_u4;
__device__ __forceinline__ gptr as_uniform_ptr(const void* p) {
    const uintptr_t v = reinterpret_cast<uintptr_t>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<gptr>(((uintptr_t)hi << 32) | lo);
}

// ---- LDS waits
__device__ __forceinline__ void as_wait_lds() {  // this wave's LDS reads are in registers, its LDS writes are done
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void as_lds_barrier() {  // LDS hazards only: unlike __syncthreads() it leaves global stores in flight
    as_wait_lds();
    __builtin_amdgcn_s_barrier();
}

// ---- DPP reductions.  The order of a sum is part of the result: a call site keeps the reduction it has.
// acc + (v of the lane that the DPP control CTRL selects)
template <int CTRL>
__device__ __forceinline__ float as_dpp_add(float acc, float v) {
    return acc + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over LPU (2 or 4) adjacent lanes (the lanes that share a hidden unit of a recurrence): quad_perm [1,0,3,2] (then [2,3,0,1])
template <int LPU>
__device__ __forceinline__ float as_quad_sum(float v) {
    v = as_dpp_add<0xB1>(v, v);
    if (LPU == 4) v = as_dpp_add<0x4E>(v, v);
    return v;
}
// Sum over the 16 lanes of a DPP row (lanes 16 k .. 16 k + 15), result in every lane of the row: four DPP steps (xor 1, xor 2,
// mirror of 8, mirror of 16: ~8 cycles each), no cross-row traffic, no v_readlane.
__device__ __forceinline__ float as_row16_sum(float v) {
    v = as_dpp_add<0xB1>(v, v);    // quad_perm [1,0,3,2]
    v = as_dpp_add<0x4E>(v, v);    // quad_perm [2,3,0,1]
    v = as_dpp_add<0x141>(v, v);   // row_half_mirror
    v = as_dpp_add<0x140>(v, v);   // row_mirror
    return v;
}
// Sum over the 64 lanes, result in every lane: the four row totals are read out with v_readlane and added as wave-uniform
// values.  (as_wave_sum's six __shfl_xor steps are six dependent LDS-crossbar round trips: 12 of them per LayerNorm row made
// lin_f32.hip's epilogue longer than the GEMM's main loop.)
__device__ __forceinline__ float as_wave_sum_dpp(float v) {
    v = as_row16_sum(v);
    const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (a + b) + (c + d);
}

// ---- closest-point scan (MeanP2CPDistance: metrics.hip, pc_eval.hip)
// min_j |p - q_j|^2 over the n points (qx, qy) in LDS (padded to a multiple of 4 with +inf coordinates): four points per
// step from two broadcast ds_read_b128, the arithmetic on float pairs (v_pk_add / v_pk_mul: half the instructions of the
// scalar form), v_min3 to fold two candidates at once.  The kernel lives on vector-instruction issue (50 x 50 pair
// distances twice per 800-byte tile), not on HBM: ~3.5 instructions per pair instead of ~8.
__device__ __forceinline__ float as_p2cp_scan(float px, float py, const float* __restrict__ qx, const float* __restrict__ qy, int n4) {
    const f32x2 px2 = {px, px}, py2 = {py, py};
    float m = INFINITY;
    for (int j = 0; j < n4; j += 4) {
        const float4 x4 = *reinterpret_cast<const float4*>(qx + j), y4 = *reinterpret_cast<const float4*>(qy + j);
        const f32x2 dxa = px2 - f32x2{x4.x, x4.y}, dxb = px2 - f32x2{x4.z, x4.w};
        const f32x2 dya = py2 - f32x2{y4.x, y4.y}, dyb = py2 - f32x2{y4.z, y4.w};
        const f32x2 sa = dxa * dxa + dya * dya, sb = dxb * dxb + dyb * dyb;
        m = fminf(fminf(m, sa.x), sa.y);
        m = fminf(fminf(m, sb.x), sb.y);
    }
    return m;
}
// The arg-min sibling (p2cp_loss.hip): the same squared distances from the same expression, so *m_out is as_p2cp_scan's
// value bit for bit, and the LOWEST index that attains it (strict < in ascending order: torch.min's tie rule).  A padding
// point (+inf) or a NaN distance is never taken; n >= 1 real points, so the index is one of theirs.
__device__ __forceinline__ int as_p2cp_scan_argmin(float px, float py, const float* __restrict__ qx, const float* __restrict__ qy, int n4,
                                                   float* __restrict__ m_out) {
    const f32x2 px2 = {px, px}, py2 = {py, py};
    float m = INFINITY;
    int at = 0;
    for (int j = 0; j < n4; j += 4) {
        const float4 x4 = *reinterpret_cast<const float4*>(qx + j), y4 = *reinterpret_cast<const float4*>(qy + j);
        const f32x2 dxa = px2 - f32x2{x4.x, x4.y}, dxb = px2 - f32x2{x4.z, x4.w};
        const f32x2 dya = py2 - f32x2{y4.x, y4.y}, dyb = py2 - f32x2{y4.z, y4.w};
        const f32x2 sa = dxa * dxa + dya * dya, sb = dxb * dxb + dyb * dyb;
        if (sa.x < m) { m = sa.x; at = j; }
        if (sa.y < m) { m = sa.y; at = j + 1; }
        if (sb.x < m) { m = sb.x; at = j + 2; }
        if (sb.y < m) { m = sb.y; at = j + 3; }
    }
    *m_out = m;
    return at;
}

// ---- exact (erf) GELU and d gelu / dx = Phi(x) + x phi(x)
__device__ __forceinline__ float as_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float as_gelu_grad(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * __expf(-0.5f * x * x);
}
