// How a head-layer descriptor finds its kernel of lin_f32.hip (lin_plan.h).  Host only: arithmetic on the descriptor and on
// as_lin_env.  A plan that declines leaves family AS_LIN_NONE and zero tiles; the caller then takes the general GEMM + row kernels.
#define AS_HOST_ONLY
#include "lin_plan.h"

#include <limits.h>

#include "as_common.h"
#include "gemm_plan.h"

namespace {

enum { EPI_PLAIN = 0, EPI_LNF = 1, EPI_LNB = 2 };
constexpr int BN = AS_LIN_BN, ON = AS_LIN_ON, BK = AS_LIN_BK, S6_BK = AS_LIN_S6_BK;
constexpr long MAX_UNITS = 1L << 30;   // 64-row tiles of a launch: the tile list then fits a grid and its fields an int

as_lin_plan declined() {
    as_lin_plan p{};
    p.family = AS_LIN_NONE;
    p.ksplit = 1;
    return p;
}

// The kernels' tile list from x, the number of 64-row tiles per batch member: those are dispatched first, then the remaining
// rows as 32-row tiles.  Every row of every member lies in exactly one tile and no tile begins at or beyond M (x <= M / 64: the
// kernels clamp a tile's rows with min(row, rows_valid - 1)).  p->tiles: the number of tiles (workgroups).
void tile_list(as_lin_plan* p, int M, int batch, long x) {
    const int rest = M - (int)x * 64;
    p->big_per_batch = x > 0 ? (int)x : 1;
    p->big_per_batch_rows = (int)x * 64;
    p->n_big = (int)(x * batch);
    p->small_per_batch = as_cdiv(rest, 32);
    p->tiles = (long)p->n_big + (long)p->small_per_batch * batch;
    if (p->small_per_batch == 0) p->small_per_batch = 1;
}

// How many 64-row tiles per batch member fill whole rounds of `slots` resident workgroups.  A launch of T equal tiles takes
// ceil(T / slots) rounds, and the head layers' 1100 tiles of 64 rows were 3 rounds of 512 of which the last held 76 tiles
// (measured: 31 us of a 118 us launch with 180 CUs idle).  So: as many 64-row tiles as fill whole rounds, dispatched first,
// then the remaining rows as 32-row tiles (half the matrix work each), which pack the last round about half as high.
// short_64: what a launch of LESS than one round gets -- false: 32-row tiles only (they spread over more CUs), true: plain
// 64-row tiles + a ragged end (the output layer: a 32-row tile loads the same W3' planes for half the rows).
long whole_round_tiles(int M, int batch, int slots, bool short_64) {
    const long units = (long)as_cdiv(M, 64) * batch;      // work in 64-row tiles
    const long rounds = units / slots;
    if (rounds == 0 && short_64) return M / 64;
    const long x = rounds * slots / batch;
    return x > M / 64 ? M / 64 : x;
}

// B as bfloat16 planes (as_emit_planes) can feed a split-arithmetic kernel whose column tile is min_rows wide: the arithmetic
// is on, K is whole 32-deep k-tiles, the image has the tile's rows, planes and batch members start 16-byte aligned, and a row
// offset of A fits the kernels' 32-bit byte offsets.  Then the kernel argument gets them; else the exact fp32 kernel
// (as_lin_plan_make, as_lin_out_plan_make) or no launch (as_lin_plain_plan_make).
template <typename L>
bool take_planes(const L* a, const as_lin_env* env, int min_rows) {
    return a->Bp && env->arith == AS_ARITH_BF16X6 && a->K % S6_BK == 0 && a->bp_rows >= min_rows && as_aligned16(a->Bp) &&
           a->bp_plane % 8 == 0 && a->bp_batch % 8 == 0 && a->lda < (1L << 23);
}

}  // namespace

void as_lin_plan_make(const as_lin* a, const as_lin_env* env, as_lin_plan* out) {
    as_lin_plan p = *out = declined();
    if (a->K % BK || a->K < BK || a->N > BN || a->N < 4 || a->M < 1 || a->batch < 1) return;
    if (!as_aligned16(a->A) || !as_aligned16(a->B) || a->lda % 4 || a->ldb % 4 || a->a_batch % 4 || a->b_batch % 4) return;
    if (!a->b_kc && a->N % 4) return;
    if (a->epi != EPI_PLAIN && (a->N != BN || !a->C)) return;
    if (a->epi == EPI_PLAIN && a->N <= BN / 2) return;  // half of the 8 feature-side waves would multiply padding
    if ((long)as_cdiv(a->M, 64) * a->batch > MAX_UNITS) return;
    if ((a->ka_valid > 0 ? a->ka_valid : a->K) % 4) return;
    if (a->epi == EPI_LNF && (!a->rstd || !a->bits || !a->b_kc)) return;
    if (a->epi == EPI_LNB && (!a->xhat || !a->rstd_in || !a->bits_in || a->b_kc)) return;
    p.epi = a->epi == EPI_LNF || a->epi == EPI_LNB ? a->epi : EPI_PLAIN;
    p.b_kc = a->b_kc != 0;
    p.planes = take_planes(a, env, BN);   // taken: the bf16 matrix instruction; else the exact fp32 kernel
    // Short reductions whose planes were taken: the kernels that keep the whole A image resident.
    const bool short_k = p.epi != EPI_PLAIN && env->short_k && p.planes && a->K <= AS_LIN_SHORT_MAXK;
    const int lds = (a->K / S6_BK) * AS_LIN_S6_IMAGE + AS_LIN_STAGE;
    if (short_k && p.epi == EPI_LNF && a->a_batch == 0 && lds <= env->lds_limit) {
        // Linear 1 (every head reads the same A): one image per row tile for a group of heads.  As many head groups as keep the
        // launch within ONE round of the 512 resident slots (at 6400 frames and 11 heads 5 groups of 2, 2, 2, 2, 3 heads x 100
        // row tiles = 500 workgroups), 64-row tiles + a ragged end unless that leaves CUs idle (fewer workgroups than 1.5 x 256:
        // 32-row tiles then).  Measured at 6400 x 11 (profiles/head_short_k_ab.log): 5 or 6 groups -4 us against lin_s6_kernel,
        // 11 groups (one head each) -1, 4 groups no gain, 3 and fewer slower -- the longest workgroup sets the time.
        const int row_tiles = as_cdiv(a->M, 64);
        const int fit = AS_LIN_SLOTS / row_tiles;
        p.family = AS_LIN_LNF_SHARED;
        p.groups = fit < 1 ? 1 : fit > a->batch ? a->batch : fit;
        p.lds = lds;
        if ((long)p.groups * a->batch > INT_MAX) return;   // the kernel finds a group's heads as t * batch / groups in 32 bits
        tile_list(&p, a->M, p.groups, (long)row_tiles * p.groups >= AS_LIN_SPREAD ? a->M / 64 : 0);   // the list counts head groups
    } else {
        // dx3 among the short reductions, and every other layer: tiles for two workgroups per CU = 512 slots (whole_round_tiles)
        p.family = short_k && p.epi == EPI_LNB ? AS_LIN_LNB_SHORT : p.planes ? AS_LIN_S6 : AS_LIN_F32;
        tile_list(&p, a->M, a->batch, whole_round_tiles(a->M, a->batch, AS_LIN_SLOTS, false));
    }
    *out = p;
}

void as_lin_plain_plan_make(const as_lin* a, int ksplit, int waves_per_simd, const as_lin_env* env, as_lin_plan* out) {
    as_lin_plan p = *out = declined();
    p.nw = a->N <= BN / 2 ? 4 : 8;
    p.wps = p.nw == 4 && waves_per_simd == 2 ? 2 : 4;   // (the 256-column kernel exists for four waves per SIMD only)
    p.planes = take_planes(a, env, p.nw * 32);
    if (!p.planes) return;
    if (a->epi != EPI_PLAIN || a->K < S6_BK || a->N > BN || a->N < 1 || a->M < 1 || a->batch < 1 || !a->C) return;
    if (!as_aligned16(a->A) || a->lda % 4 || a->a_batch % 4) return;
    const long units = (long)as_cdiv(a->M, 64) * a->batch;
    if (units > MAX_UNITS) return;
    if (ksplit == AS_LIN_KSPLIT_AUTO) {
        // dx1: as many chunks as keep the launch at <= 512 workgroups, at most two per CU, and no more than 8 slabs for the
        // consumer to add.  The slab route has only ever run on 16-byte rows (N % 4 == 0); other widths stay on the general kernel.
        if (a->N % 4) return;
        const long fit = AS_LIN_SLOTS / units;
        ksplit = fit > 8 ? 8 : (int)fit;
    }
    if (ksplit < 1) ksplit = 1;
    if (ksplit > 1 && (a->bias || a->act)) return;   // the chunks' partial sums are added by the consumer
    if ((a->ka_valid > 0 ? a->ka_valid : a->K) % 4) return;
    p.kchunk = (int)as_round_up(as_cdiv(a->K, ksplit), S6_BK);   // whole k-tiles
    p.ksplit = as_cdiv(a->K, p.kchunk);
    if (p.ksplit > 65535) return;   // grid.y
    // tiles: 64 rows unless that leaves CUs idle (fewer workgroups than 1.5 x 256)
    tile_list(&p, a->M, a->batch, units * p.ksplit >= AS_LIN_SPREAD ? a->M / 64 : 0);
    if (p.tiles > MAX_UNITS) return;
    p.family = AS_LIN_PLAIN;
    *out = p;
}

void as_lin_out_plan_make(const as_lin_out* a, const as_lin_env* env, as_lin_plan* out) {
    as_lin_plan p = *out = declined();
    if (a->K % BK || a->K < BK || a->N > ON || a->N < 4 || a->N % 2 || a->M < 1 || a->batch < 1) return;
    if (!as_aligned16(a->A) || !as_aligned16(a->B) || a->lda % 4 || a->ldb % 4 || a->a_batch % 4 || a->b_batch % 4) return;
    if (a->b_rows < a->N) return;
    if (a->tgt && (!a->lengths || !a->dout || !a->partial || a->T < 1 || a->ldo != (long)a->batch * a->N || a->o_batch != a->N)) return;
    if ((long)as_cdiv(a->M, 64) * a->batch > MAX_UNITS) return;
    // tile list as for the 256-column kernel, over rounds of 4 x 256 slots; less than one round: plain 64-row tiles.
    // The split-arithmetic kernel is built for three workgroups of a CU, not 4, and keeps this list all the same: one of
    // 3 x 256 slots (759 + 682 tiles at 6400 frames x 11 heads instead of 1023 + 154) was measured 4 us slower, as slow as
    // the kernel with scratch -- a 32-row tile loads the same W3' planes for half the rows.  (Besides, the criterion's partial
    // sums are per tile: with the list unchanged the loss is added in the order it always was.)
    tile_list(&p, a->M, a->batch, whole_round_tiles(a->M, a->batch, AS_LIN_OUT_SLOTS, true));
    if (a->tgt && p.tiles > a->partial_capacity) return;
    // the criterion's float4 rows (criterion_rows_f4): whole chunks per row, every row 16-byte aligned (ldo = batch * N)
    p.row_epi = a->tgt && env->row_epi && a->N % 4 == 0 && as_aligned16(a->out) && as_aligned16(a->dout) && as_aligned16(a->tgt);
    p.sums_loss = a->tgt && a->loss && env->counter;
    p.partials = p.sums_loss ? 0 : (int)p.tiles;   // partials that still await as_loss_final
    p.planes = take_planes(a, env, ON);
    p.family = p.planes ? AS_LIN_OUT_S6 : AS_LIN_OUT;
    *out = p;
}

bool as_linear_blocks(int N, int* bn, int* nb) {
    if (N <= 256) { *bn = N <= 128 ? 128 : 256; *nb = 1; return true; }
    if (N % 256 == 0) { *bn = 256; *nb = N / 256; return true; }
    return false;
}
