// How an as_gemm descriptor finds its kernel (gemm_plan.h).  Host only: arithmetic on the descriptor and on as_gemm_env.
//
// Order of the decision, after ALL validation:
//   1. weight-gradient shapes (both operands reduction-strided, no k_tri): gemm_s6.hip with precision == 3 and >= 256 tiles,
//      else wgrad_f32.hip (whole tiles or stream-K) where its contract holds;
//   2. forward and input-gradient shapes with precision == 3: gemm_s6.hip where its contract holds;
//   3. everything else: the general kernel on 128 x 128 tiles once they fill the chip, else on 64 x 64 tiles, either with its
//      split-K rule.
#define AS_HOST_ONLY
#include "gemm_plan.h"

#include <stdio.h>

#include "as_common.h"

namespace {

#define PLAN_REQUIRE(cond, code, ...)            \
    do {                                         \
        if (!(cond)) {                           \
            snprintf(err, err_len, __VA_ARGS__); \
            return (code);                       \
        }                                        \
    } while (0)

// gemm_s6.hip takes the descriptor (the caller has checked the arithmetic mode and precision == 3).  Forward shapes (a_k == b_k
// == 1) incl. grouped offsets (a_off ...) and relu_bits; input gradients (b_j == 1) with res / mask_bits / k_seg; weight gradients
// (a_i == b_j == 1) with colsum.  K % 16 == 0, float4-clean operands.
bool plan_s6(const as_gemm* g, as_gemm_plan* p) {
    constexpr int TB = AS_S6_TILE, BK = AS_S6_BK;
    const bool anc = g->a_k != 1;     // A[k][m], m contiguous (weight-gradient orientation)
    const bool bnc = g->b_k != 1;     // B[k][n], n contiguous (input- and weight-gradient orientation)
    if ((anc && (g->a_i != 1 || !bnc)) || (bnc && g->b_j != 1) || g->K < BK || g->K % BK || g->act > 2) return false;
    if (g->k_tri || g->accumulate || g->b_kT || g->b_kshift) return false;
    if (g->colsum && !anc) return false;
    const bool ext = g->res || g->mask_bits || g->k_seg;
    if (anc && (ext || g->relu_bits || g->bias)) return false;
    if (g->relu_bits && (g->act != 1 || ext)) return false;
    if (!anc && (g->a_i % 4 || !as_aligned16(g->A) || (!g->a_off && !g->k_seg && g->a_batch % 4))) return false;
    if (!bnc && (g->b_j % 4 || !as_aligned16(g->B) || (!g->b_off && !g->k_seg && g->b_batch % 4))) return false;
    // row-contiguous operands are loaded as float4s along the rows
    if (anc && (g->a_k % 4 || g->M % 4 || !as_aligned16(g->A) || (!g->a_off && g->a_batch % 4))) return false;
    if (bnc && (g->b_k % 4 || g->N % 4 || !as_aligned16(g->B) || (!g->b_off && !g->k_seg && g->b_batch % 4))) return false;
    if (g->k_seg && (g->k_seg % BK || g->K % g->k_seg || !g->a_seg_off || !g->b_seg_off)) return false;
    const long kspan = g->k_seg ? g->k_seg : g->K;
    // 32-bit byte offsets inside one batch member / segment
    if ((anc ? kspan * g->a_k + g->M : (long)g->M * g->a_i) >= (1L << 30) || (bnc ? kspan * g->b_k + g->N : (long)g->N * g->b_j) >= (1L << 30)) return false;
    const int tiles_m = as_cdiv(g->M, TB), tiles_n = as_cdiv(g->N, TB);
    long blocks = (long)tiles_m * tiles_n * g->batch;
    if (blocks > (1L << 30)) return false;
    int xcd_group = 0;
    if (anc) {
        // one workgroup walks the whole reduction of its tile: worth it once the tiles fill the chip (else wgrad_f32.hip's stream-K)
        if (blocks < 256) return false;
        xcd_group = tiles_m * tiles_n;
        blocks = (long)as_round_up(g->batch, 8) * xcd_group;
    } else if (tiles_n > 1) {
        blocks = (long)as_round_up((long)g->batch * tiles_m, 8) * tiles_n;
    }
    p->family = AS_GEMM_S6;
    p->tile_m = p->tile_n = TB;
    p->anc = anc; p->bnc = bnc; p->ext = ext; p->split_arith = true;
    p->vec_epi = g->N % 4 == 0 && g->ldc % 4 == 0 && as_aligned16(g->C) && (g->c_off || g->c_batch % 4 == 0) &&
                 (!g->bias || (as_aligned16(g->bias) && (g->bias_off || g->bias_batch % 4 == 0))) &&
                 (!g->res || (as_aligned16(g->res) && g->res_ld % 4 == 0 && (g->res_off || g->res_batch % 4 == 0)));
    p->xcd_group = xcd_group;
    p->work = blocks;
    return true;
}

// shape / alignment contract of one problem of wgrad_f32.hip
bool wgrad_fits(const as_gemm* g) {
    if (!(g->a_i == 1 && g->b_j == 1) || g->K < 256 || g->K % AS_WGRAD_BK || g->act != 0 || g->bias) return false;
    if (g->b_kT > 0 && (g->a_off || g->b_off || g->c_off)) return false;   // shifted operand: linear batch strides only
    if (g->M % 4 || g->N % 4 || g->a_k % 4 || g->b_k % 4 || !as_aligned16(g->A) || !as_aligned16(g->B)) return false;
    const bool grouped = g->a_off || g->b_off || g->c_off;
    if (!grouped && (g->a_batch % 4 || g->b_batch % 4)) return false;
    if ((long)g->M * g->N % 4) return false;
    return true;
}
bool wgrad_c_vec(const as_gemm* g) { return as_aligned16(g->C) && g->ldc % 4 == 0 && (g->c_off ? true : g->c_batch % 4 == 0); }

// wgrad_f32.hip takes the descriptor: 128 x 128 or 128 x 256 tiles, split over K or stream-K
bool plan_wgrad(const as_gemm* g, const as_gemm_env* env, as_gemm_plan* p) {
    if (!wgrad_fits(g)) return false;
    const int bn = g->N > 128 ? 256 : 128;
    const int tiles_m = as_cdiv(g->M, AS_WGRAD_BM), tiles_n = as_cdiv(g->N, bn);
    const long tiles = (long)tiles_m * tiles_n * g->batch;
    // too little work to give every CU a 128-row tile over >= 256 frames: the general kernel's 64 x 64 tiles spread it better
    if (tiles * (g->K / 256) < 256) return false;
    // split K so that the launch has about `target` workgroups (one per CU and round; without a cu_budget the model assumes the MI355X's 256 CUs)
    const int cus = g->cu_budget > 0 ? g->cu_budget : 256;
    long S = 1;
    const long per = (long)g->batch * g->M * g->N, per_cs = g->colsum ? (long)g->batch * g->M : 0;
    if (g->splitk_ws && tiles < cus) {
        // time ~ rounds * k-steps per workgroup * c1 + slab traffic; c1 = us per k of one 128 x bn tile on one CU
        const double c1 = (bn == 256 ? 256.0 : 128.0) / 2400.0, c2 = 8.0 / 4.0e6;  // write + read of a float at ~4 TB/s
        double best = 1e30;
        for (long s = 1; s <= 64 && s * 128 <= g->K; ++s) {
            const long chunk = as_round_up(as_cdiv(g->K, s), AS_WGRAD_BK);
            const long rounds = (tiles * s + cus - 1) / cus;
            const double cost = rounds * chunk * c1 + (s > 1 ? s * (per + per_cs) * c2 : 0.0);
            if (cost < best - 1e-9) best = cost, S = s;
        }
        if (S > g->K / 128) S = g->K / 128;
        if (S * (per + per_cs) > g->splitk_ws_floats) S = g->splitk_ws_floats / (per + per_cs);
        if (S < 1) S = 1;
    }
    p->tile_m = AS_WGRAD_BM; p->tile_n = bn;
    p->split_arith = env->arith == AS_ARITH_BF16X6;
    p->c_vec = wgrad_c_vec(g);
    // Many tiles that do not fill whole rounds of the CUs: stream-K (see WgradMulti) instead of whole tiles per workgroup
    const long rounds = (tiles + cus - 1) / cus;
    if (g->splitk_ws && tiles * 2 >= cus && tiles * 100 < rounds * cus * 95 && g->K / 32 >= 16 &&
        (long)cus * 2 * AS_WGRAD_PIECE_FLOATS <= g->splitk_ws_floats) {
        p->family = AS_GEMM_WGRAD_STREAMK;
        p->reduce = AS_REDUCE_STREAMK;
        p->nkt = g->K / 32;
        const long total_units = tiles * p->nkt;
        p->unit_per_wg = (total_units + cus - 1) / cus;
        p->work = (total_units + p->unit_per_wg - 1) / p->unit_per_wg;   // workgroups
    } else {
        p->family = AS_GEMM_WGRAD;
        p->kchunk = (int)as_round_up(as_cdiv(g->K, S), AS_WGRAD_BK);
        p->splitk = as_cdiv(g->K, p->kchunk);
        p->reduce = p->splitk > 1 ? AS_REDUCE_WGRAD : AS_REDUCE_NONE;
        p->work = (long)g->batch * p->splitk * tiles_n * tiles_m;
    }
    p->per_xcd = (int)((p->work + 7) / 8);
    return true;
}

}  // namespace

int as_gemm_plan_make(const as_gemm* g, const as_gemm_env* env, as_gemm_plan* p, char* err, size_t err_len) {
    constexpr int BK = AS_GEMM_BK;
    PLAN_REQUIRE(g && g->A && g->B && g->C, AS_ERR_BAD_ARG, "as_gemm_f32: null pointer");
    PLAN_REQUIRE(g->M > 0 && g->N > 0 && g->K > 0 && g->batch > 0, AS_ERR_BAD_ARG,
                 "as_gemm_f32: non-positive size M=%d N=%d K=%d batch=%d", g->M, g->N, g->K, g->batch);
    PLAN_REQUIRE((g->a_i == 1) != (g->a_k == 1) || (g->a_i == 1 && g->a_k == 1 && (g->M == 1 || g->K == 1)),
                 AS_ERR_BAD_ARG, "as_gemm_f32: exactly one of a_i/a_k must be 1 (a_i=%ld a_k=%ld)", (long)g->a_i, (long)g->a_k);
    PLAN_REQUIRE((g->b_j == 1) != (g->b_k == 1) || (g->b_j == 1 && g->b_k == 1 && (g->N == 1 || g->K == 1)),
                 AS_ERR_BAD_ARG, "as_gemm_f32: exactly one of b_j/b_k must be 1 (b_j=%ld b_k=%ld)", (long)g->b_j, (long)g->b_k);
    PLAN_REQUIRE(g->act >= 0 && g->act <= 3, AS_ERR_BAD_ARG, "as_gemm_f32: act=%d", g->act);
    // 3 = "the library's matrix arithmetic, at any size" (below)
    PLAN_REQUIRE(g->precision == 0 || g->precision == 3, AS_ERR_BAD_ARG, "as_gemm_f32: precision=%d (accepted: 0 and 3)", g->precision);
    // (M == 1 with both strides of A equal to 1 reads the same either way: output-contiguous then, the form the column sums take)
    const bool a_kc = g->a_k == 1 && !(g->a_i == 1 && g->colsum), b_kc = g->b_k == 1;
    PLAN_REQUIRE(!(g->b_kT > 0 && b_kc), AS_ERR_BAD_ARG, "as_gemm_f32: b_kshift needs a reduction-strided B operand");
    const long a_ld = a_kc ? g->a_i : g->a_k, b_ld = b_kc ? g->b_j : g->b_k;
    PLAN_REQUIRE(g->k_tri >= 0 && g->k_tri <= 2, AS_ERR_BAD_ARG, "as_gemm_f32: k_tri=%d", g->k_tri);
    PLAN_REQUIRE(g->k_tri == 0 || (!g->colsum && !g->splitk_ws && g->k_seg == 0 && !g->accumulate && g->act <= 1 &&
                                   !g->bias_off && (long)g->M * g->ldc < (1L << 31)),
                 AS_ERR_BAD_ARG, "as_gemm_f32: k_tri goes with the extended general kernel only (no colsum, splitk_ws, k_seg, accumulate, "
                 "act > 1)");
    const bool epi_ops = g->res || g->mask_bits || g->relu_bits, segmented = g->k_seg > 0;
    PLAN_REQUIRE(!(epi_ops || segmented) || (!g->colsum && !g->splitk_ws && !g->accumulate && (a_kc || b_kc)),
                 AS_ERR_BAD_ARG, "as_gemm_f32: res / mask_bits / relu_bits / k_seg go with the general kernel only (no colsum, splitk_ws, "
                 "accumulate or weight-gradient shape)");
    PLAN_REQUIRE(!g->relu_bits || g->act == 1, AS_ERR_BAD_ARG, "as_gemm_f32: relu_bits is the bit image of a ReLU epilogue (act == 1)");
    PLAN_REQUIRE(!(epi_ops || segmented) || (a_kc && as_aligned16(g->A) && as_aligned16(g->B) && a_ld % 4 == 0 && b_ld % 4 == 0 && g->K % 4 == 0 &&
                                             (b_kc || g->N % 4 == 0) && g->act <= 1 && (g->a_off || segmented || g->a_batch % 4 == 0) &&
                                             (g->b_off || segmented || g->b_batch % 4 == 0)),
                 AS_ERR_BAD_ARG, "as_gemm_f32: res / mask_bits / relu_bits / k_seg need a reduction-contiguous A, float4-clean operands "
                 "and act <= 1");
    PLAN_REQUIRE(!(epi_ops || segmented) || ((long)g->M * g->ldc < (1L << 31) && (long)g->M * g->res_ld < (1L << 31)),
                 AS_ERR_BAD_ARG, "as_gemm_f32: res / mask_bits / relu_bits / k_seg address one batch member's C and res with 32-bit offsets");
    PLAN_REQUIRE(!segmented || (g->k_seg % BK == 0 && g->K % g->k_seg == 0 && g->a_seg_off && g->b_seg_off && g->b_kT == 0),
                 AS_ERR_BAD_ARG, "as_gemm_f32: k_seg=%d needs a multiple of %d that divides K=%d and both segment tables", g->k_seg, BK, g->K);
    PLAN_REQUIRE(!(g->colsum && a_kc), AS_ERR_BAD_ARG, "as_gemm_f32: colsum needs an output-contiguous A operand (a_i == 1)");

    *p = as_gemm_plan{};
    p->splitk = 1; p->kchunk = g->K;
    p->a_kc = a_kc; p->b_kc = b_kc;
    const bool s6 = g->precision == 3 && env->arith == AS_ARITH_BF16X6;
    if (!a_kc && !b_kc && g->k_tri == 0) {  // weight-gradient shapes: the kernel of wgrad_f32.hip (it does not know k_tri)
        // precision == 3 in the split arithmetic: one workgroup per 128 x 128 output tile over the whole reduction, operand tiles
        // staged once per workgroup (gemm_s6.hip; the transformer's grouped weight gradients, 110 x [256 x 256 x 6400]: 704 us
        // with the stream-K kernel below, 597 - 659 us there; it declines launches of fewer than 256 tiles)
        if (s6 && g->a_i == 1 && g->b_j == 1 && plan_s6(g, p)) return 0;
        if (plan_wgrad(g, env, p)) return 0;
    }
    // precision == 3: the library's split matrix arithmetic (as_set_matrix_arith(1)) for forward shapes -- both operands
    // reduction-contiguous, plain or ReLU-bit epilogue, linear or grouped batches -- on the bf16 matrix instruction with both
    // operands split inside the kernel (gemm_s6.hip: 1.36 x this kernel on the transformer's block groups, 110 x [6400 x 256 x
    // 256]).  Opt-in per call and independent of the launch's size: a size threshold would make the last bits of a result
    // depend on the batch it was computed in (measured: 7e-5 on the transformer's contours between batches of 4 and 32).
    // The input-gradient orientation (B column-contiguous, with res / mask_bits / k_seg) goes the same way.
    if (s6 && a_kc && (b_kc || g->b_j == 1) && plan_s6(g, p)) return 0;

    const bool grouped = g->a_off || g->b_off || g->c_off || g->bias_off;
    // alignment of table offsets is the caller's contract (multiples of 4 floats) -- see header
    p->a_vec = as_aligned16(g->A) && a_ld % 4 == 0 && (grouped || segmented || g->a_batch % 4 == 0);
    p->b_vec = as_aligned16(g->B) && b_ld % 4 == 0 && (grouped || segmented || g->b_batch % 4 == 0);
    p->family = AS_GEMM_GENERAL;
    // FAST needs whole float4s: aligned operands and contiguous extents that are multiples of 4
    p->fast = p->a_vec && p->b_vec && (a_kc ? g->K % 4 == 0 : g->M % 4 == 0) && (b_kc ? g->K % 4 == 0 : g->N % 4 == 0);
    // k_tri is a hint about zeros: operands the extended (float4) instantiation cannot take run the plain kernel over the full range
    p->k_tri = g->k_tri;
    if (g->k_tri != 0 && !(as_aligned16(g->A) && as_aligned16(g->B) && a_ld % 4 == 0 && b_ld % 4 == 0 && (a_kc ? g->K % 4 == 0 : g->M % 4 == 0) &&
                           (b_kc ? g->K % 4 == 0 : g->N % 4 == 0) && (g->a_off || g->a_batch % 4 == 0) && (g->b_off || g->b_batch % 4 == 0) &&
                           (a_kc || !b_kc)))
        p->k_tri = 0;
    p->ext = epi_ops || segmented || p->k_tri != 0;   // (operands checked above: a_kc, or k_tri = 2 with both operands strided)
    const long per = (long)g->batch * g->M * (g->N + (g->colsum ? 1 : 0));   // floats of one split-K slab
    // 128x128 tiles once they fill the chip and N fills a tile (N = 100: 60 vs 72 us at 64x64), else 64x64 for more workgroups
    const long big = (long)as_cdiv(g->M, 128) * as_cdiv(g->N, 128) * g->batch;
    if (big >= 512 && g->N >= 128) {  // fewer 128x128 tiles leave most of the 768 resident slots empty: 64x64 then
                                                 // (measured 6400 x 768 x 256: 300 tiles 39.9 us, as 1200 64x64 tiles 30.1 us)
        p->tile_m = p->tile_n = 128;
        // 128x128 tiles that do not fill the resident slots (3 per CU) with a long reduction: split K so that the persistent
        // workgroups get equal shares (measured: 440 tiles, K = 6400 run at 75 TF/s, 768 tiles of the same shape at 100)
        const int slots = env->slots128;
        if (g->splitk_ws && !grouped && big < slots && g->K >= 2048 && !g->bias && g->act == 0) {
            long best = 1;
            double best_cost = 1.0;  // rounds of work per workgroup, in units of the unsplit tile time
            for (long sk = 2; sk <= 8 && sk * per <= g->splitk_ws_floats; ++sk) {
                const double cost = (double)((big * sk + slots - 1) / slots) / sk + 0.02 * sk;  // + slab traffic
                if (cost < best_cost - 1e-9) best_cost = cost, best = sk;
            }
            if (best > 1) {
                p->kchunk = (int)as_round_up(as_cdiv(g->K, best), BK);
                p->splitk = as_cdiv(g->K, p->kchunk);
                p->reduce = AS_REDUCE_SPLITK;
            }
        }
        if (p->splitk == 1) p->xcd_panels = a_kc && g->N > 128 && g->k_tri == 0 && big >= 2048 && slots % 8 == 0;
        p->work = big * p->splitk;
        return 0;
    }
    p->tile_m = p->tile_n = 64;
    // few output tiles and a long reduction (weight gradients): split K over workgroups
    const long tiles = (long)as_cdiv(g->M, 64) * as_cdiv(g->N, 64) * g->batch;
    if (g->splitk_ws && !grouped && tiles < 512 && g->K >= 512 && !g->bias && g->act == 0) {
        long sk = (1024 + tiles - 1) / tiles;
        const int min_chunk = tiles * (g->K / 128) < 128 ? 64 : 128;  // a handful of tiles: shorter chunks, still >= 2 k-steps
        if (sk > g->K / min_chunk) sk = g->K / min_chunk;
        if (sk > 64) sk = 64;
        if (sk * per > g->splitk_ws_floats) sk = g->splitk_ws_floats / per;
        // weight-gradient shapes with many tiles per chunk: a multiple of 8 chunks, one XCD per chunk (GemmK::xcd_chunks)
        const bool want_xcd = !a_kc && !b_kc && sk >= 12 && tiles >= 16;
        if (want_xcd)   // the nearest multiple of 8 (downwards) whose BK-rounded chunks still number a multiple of 8
            for (long c = (sk + 4) / 8 * 8; c >= 8; c -= 8)
                if (as_cdiv(g->K, as_round_up(as_cdiv(g->K, c), BK)) % 8 == 0) { sk = c; break; }
        if (sk > 1) {
            p->kchunk = (int)as_round_up(as_cdiv(g->K, sk), BK);
            p->splitk = as_cdiv(g->K, p->kchunk);
            p->xcd_chunks = want_xcd && p->splitk % 8 == 0;
        }
        if (p->splitk > 1) {
            // many slabs over few outputs: the four-way reduce kernel; one shape always takes the same kernel
            const int wide = p->splitk >= 16 && per <= (1L << 20) ? AS_REDUCE_SPLITK4 : AS_REDUCE_SPLITK;
            // few slabs: the last workgroup to arrive at a tile sums them in the kernel (input gradient of GRU layer 1, 3 slabs:
            // 52 us against 36 + 45 for a reduce kernel that has to squeeze in beside the side stream's persistent GEMM).
            // Many slabs (a handful of tiles) would leave the sums to a handful of workgroups: the wide reduce kernel then.
            const bool arrive = p->splitk <= 16 && tiles < env->counters;
            p->reduce = arrive ? AS_REDUCE_COUNTERS : wide;
            p->reduce_fallback = arrive ? wide : AS_REDUCE_NONE;
        }
    }
    p->work = tiles * p->splitk;
    return 0;
}

// Chunk length of a multi-problem weight-gradient launch: every problem runs on 128 x 256 tiles and is split over K in chunks
// of the same length, chosen so that the grid is a few rounds of the CUs the caller expects (cu_budget, 0 = chip): many short
// workgroups instead of one long one per CU, so the dispatcher fills every free CU and other streams' kernels get CUs as
// workgroups retire.
bool as_wgrad_multi_plan_make(const as_wgrad_job* jobs, int n, long slab_floats, int cu_budget, as_wgrad_multi_plan* p) {
    if (n < 1 || n > AS_WGRAD_MAXP) return false;
    long tiles = 0;
    const int K = jobs[0].g.K;
    for (int i = 0; i < n; ++i) {
        const as_gemm* g = &jobs[i].g;
        if (g->K != K || g->a_off || g->b_off || g->c_off || !wgrad_fits(g)) return false;
        if (jobs[i].colsum_b && g->b_kT > 0) return false;
        tiles += (long)as_cdiv(g->M, AS_WGRAD_BM) * as_cdiv(g->N, 256) * g->batch;
    }
    // chunk length: a multiple of 32 frames, at least 256; cost = rounds of `cus` workgroups x (chunk + fixed cost per
    // workgroup) + slab traffic, all in units of one k-tile of 32 frames (~4 us for a 128 x 256 tile)
    const int cus = cu_budget > 0 ? cu_budget : 256;
    const int nkt = K / 32;
    int best_chunk = nkt;
    double best = 1e30;
    for (int chunk = 8; chunk <= nkt; ++chunk) {
        const long S = as_cdiv(nkt, chunk);
        const long W = tiles * S;
        const double rounds = (double)((W + cus - 1) / cus);
        const double cost = rounds * (chunk + 1.0) + 0.016 * W;   // 128 KB of slab written + read per workgroup at ~4 TB/s
        if (cost < best - 1e-9) best = cost, best_chunk = chunk;
    }
    *p = as_wgrad_multi_plan{};
    p->kchunk = best_chunk * 32;
    p->splitk = as_cdiv(K, p->kchunk);
    long off_f = 0, item0 = 0, red0 = 0;
    for (int i = 0; i < n; ++i) {
        const as_gemm* g = &jobs[i].g;
        const long per = (long)g->batch * g->M * g->N;
        const long per_cs = g->colsum ? (long)g->batch * g->M : 0, per_csb = jobs[i].colsum_b ? (long)g->batch * g->N : 0;
        p->c_vec[i] = wgrad_c_vec(g);
        p->slab_off[i] = off_f;
        if (p->splitk > 1) off_f += as_round_up((long)p->splitk * (per + per_cs + per_csb), 64);
        p->item0[i] = item0;
        p->red0[i] = red0;
        item0 += (long)g->batch * p->splitk * as_cdiv(g->N, 256) * as_cdiv(g->M, AS_WGRAD_BM);
        red0 += per / 4 + per_cs + per_csb;
    }
    if (off_f > slab_floats) return false;
    p->total_items = item0;
    p->total_red = red0;
    p->per_xcd = (int)((item0 + 7) / 8);
    return true;
}
