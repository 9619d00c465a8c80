// Internal (non-ABI) hand-over between the GEMM translation units.
#pragma once
#include "as_common.h"
#include "gemm_plan.h"
#include "lin_plan.h"

// The launchers as_gemm_f32 switches into once gemm_plan.cpp has validated the descriptor and chosen the kernel: each copies
// descriptor fields into its kernel-argument struct and picks the instantiation from the plan.  0, or a launch error.
int as_gemm_s6_launch(const as_gemm* g, const as_gemm_plan& p, hipStream_t st);   // gemm_s6.hip
int as_wgrad_launch(const as_gemm* g, const as_gemm_plan& p, hipStream_t st);     // wgrad_f32.hip
// wgrad_f32.hip: several weight-gradient problems as one launch (as_wgrad_job, gemm_plan.h).  1 = launched, 0 = not a case
// (caller falls back), < 0 = error.
// exact: the fp32 matrix instruction whatever as_matrix_arith() says -- for launches that run BESIDE a latency-bound kernel: the
// bf16 instruction draws more power, the chip clocks ~10 % lower under it, and a recurrence on the other CUs pays that on
// every dependent step (measured in the BiGRU step: weight gradients 161 -> 114 us, the recurrence beside them 115 -> 131 us).
int as_wgrad_multi(const as_wgrad_job* jobs, int n, float* slab, long slab_floats, int cu_budget, hipStream_t st, bool exact = false);

int as_matrix_arith();   // error.cpp: AS_ARITH_FP32 or AS_ARITH_BF16X6 (gemm_plan.h)

// rowops.hip: B[batch][n][k] (element strides n_stride, k_stride, batch_stride) as three bfloat16 planes
// out[plane][batch][Kpad / 16][rows_pad][16] (x = hi + mid + lo exactly; n >= N or k >= K: zeros).  Up to 8 jobs, one launch.
struct as_planes_job {
    const float* B; long n_stride, k_stride, batch_stride;
    int batch, N, K, rows_pad, Kpad;
    uint16_t* out;      // plane stride = batch * (Kpad / 16) * rows_pad * 16 elements, batch stride = (Kpad / 16) * rows_pad * 16
};
int as_emit_planes(const as_planes_job* jobs, int n, hipStream_t st);
static inline long as_planes_batch_stride(int rows_pad, int Kpad) { return (long)(Kpad / 16) * rows_pad * 16; }
static inline long as_planes_floats(int batch, int rows_pad, int Kpad) { return 3 * batch * as_planes_batch_stride(rows_pad, Kpad) / 2; }

// A cross-stream fork without a barrier packet on the producing stream: the event is bound to the completion of the NEXT kernel
// this thread launches through a launch site that knows the mechanism (hipExtLaunchKernelGGL's stopEvent: the dispatch packet's
// own completion signal), instead of hipEventRecord's marker packet behind it (~7 us on the stream that records it, measured on
// the step timeline).  as_stop_event_take(): the event if no launch has consumed it (the caller then records it the ordinary way).
void as_stop_event_set_raw(void* ev);
void* as_stop_event_take_raw();
inline void as_stop_event_set(hipEvent_t ev) { as_stop_event_set_raw((void*)ev); }
inline hipEvent_t as_stop_event_take() { return (hipEvent_t)as_stop_event_take_raw(); }

// lin_f32.hip: the head layers (descriptors and the planner that picks each kernel: lin_plan.h).  Every entry point makes its
// plan and launches what the plan names: 1 = launched, 0 = not a case for these kernels (take the general GEMM + row kernels),
// < 0 = error.
// What the planner reads besides the descriptor, as of now.  ask_counter: also whether the stream has an arrival counter
// (asking creates it: only the output layer with a loss to sum asks).
as_lin_env as_lin_env_of(hipStream_t st, bool ask_counter = false);
int as_lin_try(const as_lin* a, hipStream_t st);
// epi 0 on the bf16 matrix instruction (a->Bp required; a->B unused): C = act(A . B^T + bias), N <= 256, K % 32 == 0.
// ksplit > 1: the reduction is cut into chunks, chunk y writes its partial sums (no bias / activation allowed) to
// C + y * c_split floats; the CONSUMER adds the slabs.  How many chunks there really are, as_lin_plain_plan_make says ahead of
// the launch (as_lin_plan.ksplit; ksplit = AS_LIN_KSPLIT_AUTO: the planner's own split for the heads' dx1).
// waves_per_simd: 4, or 2 for a launch (N <= 128) that never has more than three workgroups of a CU resident: the instantiation
// with registers for the whole 64-row loop (same instructions per accumulator: same result, bit for bit).
int as_lin_plain_s6(const as_lin* a, int ksplit, long c_split, hipStream_t st, int waves_per_simd = 4);
// the heads' output layer.  Fused criterion: *n_partials workgroup sums were written to `partial` and await as_loss_final; 0 of
// them when the kernel has summed them into a->loss itself.
int as_lin_out_try(const as_lin_out* a, int* n_partials, hipStream_t st);
// gemm_f32.hip: one of the stream's arrival counters (a device word that every launch leaves zero), or nullptr
int* as_arrival_counter(hipStream_t st);
// metrics.hip: *loss = scale * sum of the first n partials (fixed order)
int as_loss_final(const float* partial, int n, float scale, float* loss, hipStream_t st);

// gru.hip: backward recurrence of layer 0 under a token table; see the kernel.  1 = launched, 0 = not a case, < 0 = error.
bool as_gru_bwd_tokens_fits(int32_t V, int32_t H, int32_t T);   // the [V][3H] table + T offsets fit the kernel's LDS budget
int as_gru_bidir_bwd_tokens(const float* dy, const float* y, const float* gates, const float* w_hh, const int32_t* lengths,
                            int32_t B, int32_t T, int32_t H, float* dgh, const int64_t* tokens, int64_t tok_stride, int32_t V,
                            float* part, hipStream_t st);
// gru.hip: as_gru_bidir_fwd over a token table [V][2][3H] with the ids clamped into [0, V) (memory safety; the composite
// entry point counts out-of-range ids for the host)
int as_gru_bidir_fwd_tokens(const float* table, const int64_t* tokens, int64_t tok_stride, int32_t V, const float* w_hh,
                            const float* b_hh, const int32_t* lengths, int32_t B, int32_t T, int32_t H, float* y, float* gates,
                            hipStream_t st);
// rowops.hip: *count = number of ids outside [0, V) among tokens[b][t], b < rows / T, t < T (one small workgroup)
int as_count_bad_tokens(const int64_t* tokens, long tok_stride, int T, long rows, int V, int* count, hipStream_t st);
// rowops.hip: out[i] = sum over chunks (fixed order) of part[chunk][i], i < n
int as_sum_partials(const float* part, long n, int chunks, float* out, hipStream_t st);
