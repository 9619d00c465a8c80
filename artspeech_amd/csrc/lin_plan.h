// Which kernel of lin_f32.hip a head-layer descriptor gets, with what tile list, LDS and k-split: the one place that decides
// (lin_plan.cpp).  Plain C++17 on the descriptors and on as_lin_env; no HIP, no globals, no caches -- it compiles and runs on a
// machine without a GPU (tests/test_lin_plan_host.py).  The launchers in lin_f32.hip (as_lin_try, as_lin_plain_s6,
// as_lin_out_try) fill the environment, make the plan, copy descriptor and plan fields into their kernel-argument structs and
// launch the instantiation the plan names; none of them tests a shape.
#pragma once
#include <stdint.h>

// tile geometry of lin_f32.hip, as far as the choice depends on it (the file asserts its own constants against these)
constexpr int AS_LIN_BN = 256, AS_LIN_ON = 128;        // columns of a workgroup: the head layers' kernels, the output layer's
constexpr int AS_LIN_BK = 16, AS_LIN_S6_BK = 32;       // depth of a k-tile: the exact fp32 kernels, the split-arithmetic ones
constexpr int AS_LIN_SHORT_MAXK = 128;                 // S6R_MAXK: the longest reduction whose whole A image stays resident
constexpr int AS_LIN_S6_IMAGE = 12 * 1024;             // bytes of the A plane image per k-tile (3 planes x 64 rows x 32 bf16)
constexpr int AS_LIN_STAGE = 32 * 1024;                // bytes of the LayerNorm epilogue's staging area (32 rows x 256 floats)
constexpr int AS_LIN_SLOTS = 512, AS_LIN_OUT_SLOTS = 1024;   // resident workgroups: two per CU (head layers), four (output layer)
constexpr int AS_LIN_SPREAD = 384;                     // fewer 64-row workgroups than 1.5 x 256 CUs leave CUs idle: 32-row tiles then
constexpr int AS_LIN_LDS_MI355X = 160 * 1024;          // dynamic LDS a workgroup can have on the MI355X

// ---- the descriptors.  Strides in floats (planes: in bf16 elements).
// One Linear of the ArticulatorPredictor heads with the adjoining LayerNorm fused in (batched over heads):
//   C[bz] = epilogue(A[bz] [M][K] . B[bz]),  B[bz] = [N][K] (b_kc: forward) or [K][N] (backward); N <= 256, K % 32 == 0.
//   epi 0: act(. + bias) (act as as_gemm: 0 none, 1 ReLU, 2 sigmoid)
//   epi 1: x = relu(. + bias); C = (x - mean) * rstd over the 256 features; rstd [M][batch]; bits [M][batch][4] = x > 0
//   epi 2: g = .; C = relu'(bits_in) * rstd_in * (g - mean g - xhat * mean(g xhat))   (LayerNorm + ReLU backward)
// ka_valid (0 = K): k >= ka_valid of A is not read (the caller's B has zero rows there).
struct as_lin {
    const float* A; long lda, a_batch;
    const float* B; long ldb, b_batch; int b_kc;
    // optional: the same B as three bfloat16 planes [plane][batch][K / 16][bp_rows][16] (as_emit_planes; rows >= N zero,
    // strides in bf16 elements).  With as_matrix_arith() == AS_ARITH_BF16X6 and K % 32 == 0 the layer then runs on the bf16
    // matrix instruction (six plane products per fp32 product, fp32 accumulate: lin_s6_kernel); B itself is not read.
    const uint16_t* Bp; long bp_plane, bp_batch; int bp_rows;
    float* C; long ldc, c_batch;
    const float* bias; long bias_batch;
    int M, N, K, ka_valid, batch, act, epi;
    float* rstd; unsigned long long* bits;
    const float* xhat; long ldx, x_batch; const float* rstd_in; const unsigned long long* bits_in;
};
// The heads' output layer out[M][batch][N] = sigmoid(A[M][batch][K] . B[batch][>= 128 rows][K]^T + bias), N <= 128,
// optionally with the masked Euclidean criterion fused (tgt != NULL): loss partials (one per workgroup, `partial`, at most
// partial_capacity) and d loss / d(pre-sigmoid) in `dout` (layout of out).
struct as_lin_out {
    const float* A; long lda, a_batch;
    const float* B; long ldb, b_batch; int b_rows;
    const float* bias; long bias_batch;
    float* out; long ldo, o_batch;
    int M, N, K, batch;
    const float* tgt; long tgt_T; const int* lengths; int T; float scale;
    float* dout; float* partial; long partial_capacity;
    const uint16_t* Bp; long bp_plane, bp_batch; int bp_rows;   // optional: B as bfloat16 planes, bp_rows >= 128 (see as_lin.Bp)
    // optional with tgt: the device scalar that receives scale * sum of the partials.  The workgroup that delivers the LAST partial
    // adds them all itself, in the order of as_loss_final (same value): no second launch on the critical stream.  Needs an arrival
    // counter (as_arrival_counter); without one the partials are left for as_loss_final as before (*n_partials > 0).
    float* loss;
};

// what the decisions read besides the descriptor; the launcher fills it at each call
struct as_lin_env {
    int arith;        // as_matrix_arith(): AS_ARITH_FP32 (0) or AS_ARITH_BF16X6 (1), gemm_plan.h
    bool short_k;     // as_set_head_short_k: the resident-image kernels for K <= 128
    bool row_epi;     // as_set_lin_out_row_epilogue: the criterion's float4 rows
    bool counter;     // the stream has an arrival counter (as_arrival_counter(st) != nullptr)
    int lds_limit;    // dynamic LDS bytes a workgroup can have
};

enum as_lin_family {
    AS_LIN_NONE,           // declined: nothing is launched, the caller takes the general route
    AS_LIN_F32,            // lin_f32_kernel<64, b_kc, epi>
    AS_LIN_S6,             // lin_s6_kernel<epi>
    AS_LIN_LNF_SHARED,     // lin_s6_lnf_shared_kernel
    AS_LIN_LNB_SHORT,      // lin_s6_lnb_short_kernel
    AS_LIN_PLAIN,          // lin_s6_plain_kernel<nw, wps>
    AS_LIN_OUT,            // lin_out_kernel
    AS_LIN_OUT_S6,         // lin_out_s6_kernel
};

// everything a launch needs besides pointers
struct as_lin_plan {
    int family;
    bool planes;                 // the bfloat16 planes go into the kernel argument
    bool b_kc; int epi;          // AS_LIN_F32 / AS_LIN_S6: the instantiation
    int nw, wps;                 // AS_LIN_PLAIN: column waves (4: 128 columns, 8: 256) and waves per SIMD the instantiation is built for
    // the tile list: n_big tiles of 64 rows first (big_per_batch per batch member, covering big_per_batch_rows rows), then tiles
    // of 32 rows (small_per_batch per member) over the remaining rows; `tiles` workgroups in all.  The two divisors are >= 1.
    int n_big, big_per_batch, big_per_batch_rows, small_per_batch;
    long tiles;
    int groups;                  // AS_LIN_LNF_SHARED: head groups (the tile list then counts groups, not heads); else 0
    int lds;                     // dynamic LDS bytes
    int ksplit, kchunk;          // AS_LIN_PLAIN: grid.y and the k-chunk of each (whole 32-deep k-tiles); else 1 and 0
    bool row_epi;                // output layer: the criterion runs through criterion_rows_f4
    bool sums_loss;              // output layer: the last workgroup adds the partials into as_lin_out.loss (arrival counter)
    int partials;                // output layer: partials left for as_loss_final
};

// Each fills *p; p->family == AS_LIN_NONE: not a case for these kernels.
void as_lin_plan_make(const as_lin* a, const as_lin_env* env, as_lin_plan* p);
// ksplit: chunks of the reduction asked for (the plan says how many there are: whole 32-deep k-tiles each), or
// AS_LIN_KSPLIT_AUTO: the heads' dx1, a few tiles under a long reduction whose slabs the caller's LayerNorm backward adds
constexpr int AS_LIN_KSPLIT_AUTO = 0;
void as_lin_plain_plan_make(const as_lin* a, int ksplit, int waves_per_simd, const as_lin_env* env, as_lin_plan* p);
void as_lin_out_plan_make(const as_lin_out* a, const as_lin_env* env, as_lin_plan* p);

// Column blocks of the plain kernel for an N-column Linear (as_linear_fwd): block width (rows of the plane image) and count;
// false: N is neither one block nor whole 256-column blocks
bool as_linear_blocks(int N, int* bn, int* nb);
