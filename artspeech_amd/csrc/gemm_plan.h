// Which kernel an as_gemm descriptor gets, and with what grid: the one place that decides (gemm_plan.cpp).  Plain C++17 on the
// descriptor, the arithmetic mode and two facts about the device and the stream (as_gemm_env); no HIP, no globals, no caches --
// it compiles and runs on a machine without a GPU (tests/test_gemm_plan_host.py).  The launchers in gemm_f32.hip, gemm_s6.hip and
// wgrad_f32.hip copy descriptor fields into their kernel-argument structs and pick the template instantiation from the plan; none
// of them tests a shape or declines.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "artspeech_hip.h"

// How fp32 matrix products are formed (as_set_matrix_arith, include/artspeech_hip.h):
//   AS_ARITH_FP32    v_mfma_f32_32x32x2_f32 on the fp32 operands (every kernel has this path)
//   AS_ARITH_BF16X6  operands split exactly into three bfloat16 planes, six plane products on v_mfma_f32_32x32x16_bf16,
//                    fp32 accumulation -- where a kernel has the path (the default)
enum { AS_ARITH_FP32 = 0, AS_ARITH_BF16X6 = 1 };

// tile geometry of the kernels, as far as the choice depends on it (each kernel file asserts its own constants against these)
constexpr int AS_GEMM_BK = 32;                        // gemm_f32.hip: depth of a k-tile
constexpr int AS_S6_TILE = 128, AS_S6_BK = 16;        // gemm_s6.hip: square output tile, depth of a k-tile
constexpr int AS_WGRAD_BM = 128, AS_WGRAD_BK = 32;    // wgrad_f32.hip: tile rows (columns: 128 or 256), depth of a k-tile
constexpr int AS_WGRAD_PIECE_FLOATS = AS_WGRAD_BM * 256 + AS_WGRAD_BM + 256;   // a stream-K piece: tile + both column sums

// what the launch code knows about the device and the stream.  The CU count is NOT among it: the weight-gradient rules count in
// as_gemm.cu_budget, or in the MI355X's 256 CUs where the caller gives none (a constant, as before the planner existed), and the
// general kernel's rules count in resident slots.
struct as_gemm_env {
    int arith;      // as_matrix_arith()
    int slots128;   // resident workgroups of gemm_f32_kernel<128, 128, true, true, true> on the whole device (3 per CU: 768)
    int counters;   // words of the stream's arrival-counter block the split-K kernel may use (0: none)
};

enum as_gemm_family {
    AS_GEMM_GENERAL,         // gemm_f32.hip: gemm_f32_kernel<tile, tile, a_kc, b_kc, fast | ext>
    AS_GEMM_S6,              // gemm_s6.hip:  gemm_s6_kernel<anc, bnc, ext>
    AS_GEMM_WGRAD,           // wgrad_f32.hip: wgrad_f32_kernel<tile_n, false, split_arith>, whole tiles per workgroup
    AS_GEMM_WGRAD_STREAMK,   // wgrad_f32.hip: wgrad_f32_kernel<tile_n, true, split_arith>
};
enum as_gemm_reduce {
    AS_REDUCE_NONE,
    AS_REDUCE_COUNTERS,      // in the kernel, by the last workgroup to arrive at a tile (needs the stream's counter block)
    AS_REDUCE_SPLITK,        // splitk_reduce_kernel
    AS_REDUCE_SPLITK4,       // splitk_reduce4_kernel
    AS_REDUCE_WGRAD,         // wgrad_reduce_kernel
    AS_REDUCE_STREAMK,       // wgrad_reduce_sk_kernel
};

// everything a launcher needs besides pointers
struct as_gemm_plan {
    int family;
    int tile_m, tile_n;          // output tile of a workgroup
    bool a_kc, b_kc;             // general kernel: the operand is reduction-contiguous
    bool anc, bnc;               // gemm_s6: the operand is row-contiguous (X[k][row])
    bool fast, ext;              // general kernel: whole-float4 loads; the instantiation with res / mask_bits / relu_bits / k_seg / k_tri
    bool split_arith;            // the products run on the bf16 matrix instruction in the library's split arithmetic
    bool a_vec, b_vec, c_vec, vec_epi;
    int k_tri;                   // as_gemm.k_tri, or 0 where the hint cannot be used
    int splitk, kchunk;
    int reduce;                  // as_gemm_reduce
    int reduce_fallback;         // reduce == AS_REDUCE_COUNTERS and the stream has no counter block: this kernel instead
    int xcd_panels, xcd_chunks, xcd_group;
    int nkt, per_xcd;            // weight-gradient kernels: k-tiles of the reduction (stream-K); work items per XCD
    long unit_per_wg;            // stream-K: k-tile units per workgroup
    long work;                   // work items of the launch (stream-K: workgroups); a persistent kernel's launcher clamps its grid to
                                 // its resident slots, the weight-gradient launchers round up to 8 * per_xcd
};

// 0 and *p, or an AS_ERR_* code and the as_last_error() text in err.  Nothing is launched by anyone before this has returned 0.
int as_gemm_plan_make(const as_gemm* g, const as_gemm_env* env, as_gemm_plan* p, char* err, size_t err_len);

// Several weight-gradient problems of the same reduction length (a_i == b_j == 1, linear batch strides, N > 128) as ONE
// launch of 128 x 256 tiles + one reduce launch.  g.splitk_ws / cu_budget of the jobs are ignored (slab, cu_budget here).
// colsum_b (optional): column sums of the B operand [batch][N] (the bias gradient when the problem is posed transposed);
// c_trans: the result is stored transposed, C[batch][n * ldc + m].
struct as_wgrad_job {
    as_gemm g;
    float* colsum_b; long colsum_b_batch;
    int c_trans;
};
constexpr int AS_WGRAD_MAXP = 6;   // problems per launch
struct as_wgrad_multi_plan {
    int kchunk, splitk;            // the same for every problem
    bool c_vec[AS_WGRAD_MAXP];
    long slab_off[AS_WGRAD_MAXP];  // first float of the problem's slabs (C, then column sums of A, then of B)
    long item0[AS_WGRAD_MAXP], red0[AS_WGRAD_MAXP];   // first work item / first reduce thread of the problem
    long total_items, total_red;
    int per_xcd;
};
// true and *p, or false: not a case (the caller issues the problems one by one)
bool as_wgrad_multi_plan_make(const as_wgrad_job* jobs, int n, long slab_floats, int cu_budget, as_wgrad_multi_plan* p);
