// Linear layers of the ArticulatorPredictor heads (encoder_decoder/models.py:10-33) with their LayerNorms fused into the
// GEMM that produces (forward) or consumes (backward) the normalised activations:
//
//   forward   x_hat_next = LN(relu(x_hat . W'^T + b'))        C = A[M][K] . B[N][K]^T   (B reduction-contiguous, "NT")
//   backward  dz = relu' * LNbwd(dz_next . W')                 C = A[M][K] . B[K][N]     (B output-contiguous, "NN")
//
// (W', b' = the weights with the LayerNorm affine folded in; LN = affine-free normalisation over the 256 features of one
// head.)  Unfused, every such layer moves its [rows][A][256] activation through HBM three to five times (GEMM store,
// normalize load + store, and in the backward x_hat besides): 216-288 MB per layer at B*T = 6400 against 72-144 MB here.
//
// One workgroup owns BM = 64 frames x the 256 features of ONE head, so a row's LayerNorm statistics never leave the
// workgroup.  8 waves side by side along the features (32 columns x all 64 rows each: two accumulators).  60 KB of LDS and
// < 128 VGPRs: TWO workgroups per CU, so that one's prologue (DMA latency), barriers and epilogue (a pure memory phase:
// 64 KB of x_hat out, in the backward 64 KB in as well) run under the other's MFMAs.  (One 96/128-row workgroup per CU with
// a deeper ring was measured first: every CU reached its epilogue at the same moment, 35-43 us of a 130 us launch were
// epilogue with the matrix pipes idle.)
// Operands stream through a 3-slot LDS ring of 16-deep k-tiles filled by LDS-DMA (global_load_lds_dwordx4, two k-tiles in
// flight, counted vmcnt + raw barriers) like wgrad_f32.hip.  Reduction-contiguous operands keep their global layout in LDS
// ([row][16 k], no padding possible under DMA) with the four 16-byte chunks of a row XOR-swizzled by (row >> 2) & 3 on the
// SOURCE address: a lane then takes four consecutive k of its row with ONE conflict-free ds_read_b128, which feed four
// MFMA k-steps (k-step j of an 8-group pairs k = j in lanes 0-31 with k = j + 4 in lanes 32-63, for both operands alike).
// Epilogue, 32 rows at a time: the accumulators go to LDS (the ring's memory), then one wave per row does exactly what
// normalize_fwd_kernel / normalize_bwd_kernel (rowops.hip) do, reading the GEMM result from LDS instead of HBM.
//
// The file, top to bottom: what the kernels share around their main loops, each written once (tile_of: tile-list decode,
// Stamps: debug stamps, store_rows: the plain store); the LayerNorm epilogues; lin_f32_kernel (exact fp32, described above); the
// split-arithmetic main loop s6_main_loop, its entry s6_tile, and lin_s6_kernel on it; the short reductions (K <= 128: the whole
// A image resident, s6_resident_loop without barriers; lin_s6_lnf_shared_kernel = Linear 1, one image per row tile for a group
// of heads, lin_s6_lnb_short_kernel = dx3); lin_s6_plain_kernel; the output layer (criterion_rows: the fused criterion,
// criterion_rows_f4: the same through float4 rows; lin_out_kernel, lin_out_s6_kernel); the host half (the kernels' constants
// asserted against lin_plan.h, the two switches as_set_head_short_k and as_set_lin_out_row_epilogue, argument copies, and
// as_lin_try, as_lin_plain_s6, as_lin_out_try, as_linear_fwd: each makes its plan in lin_plan.cpp and launches what the plan
// names).  The kernels differ in their main loops and in which of the shared pieces they call.
#include <cstdlib>

#include <atomic>
#include <type_traits>

#include "as_launch.h"
#include "gemm_internal.h"
#include "split_arith.h"

namespace {

constexpr int BN = 256, BK = 16, NT = 512, NBUF = 3;
enum { EPI_PLAIN = 0, EPI_LNF = 1, EPI_LNB = 2 };

struct LinK {
    const float* A; long lda, a_batch;
    const float* B; long ldb, b_batch;
    const uint16_t* Bp; long bp_plane, bp_batch; int bp_rows;   // lin_s6_kernel: B as three bfloat16 planes (as_lin.Bp)
    int kchunk; long c_split;           // lin_s6_plain_kernel: blockIdx.y = k-chunk of kchunk, its partial result at C + y * c_split
    float* C; long ldc, c_batch;
    const float* bias; long bias_batch;
    int M, N, K, ka_valid, batch, act;
    int n_big, big_per_batch, big_per_batch_rows, small_per_batch;   // tiles of 64 rows first, then tiles of 32 rows (see tile_list())
    int groups;                       // lin_s6_lnf_shared_kernel: head groups (the tile list then counts groups, not heads)
    unsigned long long* dbg; long dbg_max;   // diagnostic cycle stamps (as_lin_debug_stamps), normally null
    float eps;
    float* rstd;                      // EPI_LNF out: [M][batch]
    unsigned long long* bits;         // EPI_LNF out: [M][batch][4]: v > 0 per feature
    const float* xhat; long ldx, x_batch;   // EPI_LNB in: the normalised activations this layer's LayerNorm produced
    const float* rstd_in;             // EPI_LNB in: [M][batch]
    const unsigned long long* bits_in;
};

// ---- what the five kernels share besides their main loops: the tile decode, the debug stamps, the plain store.
// A workgroup's entry of the tile list (tile_list(), lin_plan.cpp; LinK and LinOutK name its fields alike): the 64-row tiles of every
// head first, then 32-row tiles over the remaining rows of every head.  Block b takes entry b (an XCD-contiguous map --
// workgroups go to the eight XCDs round-robin by block index, each with its own 4 MB L2; XCD x took a contiguous range of
// the list, two or three heads' weights per L2 instead of all eleven -- was measured: 5-10 % slower).
// UNIFORM (the split-arithmetic kernels): the divisions run on the vector unit, and without readfirstlane head and first row
// (and their 64-bit forms) sit in vector registers from here to the epilogue; lin_s6_kernel<EPI_LNB>, at its register limit
// in the main loop, spills them.
struct Tile { int bz, m0, tm; };   // head, first row, row blocks of 32 (2 | 1)
template <bool UNIFORM, typename K>
__device__ __forceinline__ Tile tile_of(const K& g) {
    const int tile = blockIdx.x;
    Tile t;
    if (tile < g.n_big) {
        t.bz = tile / g.big_per_batch;
        t.m0 = (tile - t.bz * g.big_per_batch) * 64;
        t.tm = 2;
    } else {
        const int j = tile - g.n_big;
        t.bz = j / g.small_per_batch;
        t.m0 = g.big_per_batch_rows + (j - t.bz * g.small_per_batch) * 32;
        t.tm = 1;
    }
    if (UNIFORM) {
        t.bz = __builtin_amdgcn_readfirstlane(t.bz);
        t.m0 = __builtin_amdgcn_readfirstlane(t.m0);
    }
    return t;
}

// Diagnostic cycle stamps (as_lin_debug_stamps, tools/lin_stamps.py), normally off: thread 0 of each of the first dbg_max
// workgroups fills eight 64-bit slots.  s_memtime: 0 start, 1 first k-tile staged, 2 main loop done, 3 epilogue stored;
// s_memrealtime: 4 start, 6 end (0 until then); 5: hardware ids (s_getreg: HW_ID bits 0-3 | XCC_ID << 32).
struct Stamps {
    unsigned long long* dbg;
    bool on;
    __device__ __forceinline__ Stamps(const LinK& g, int tid) : dbg(g.dbg), on(g.dbg != nullptr && tid == 0 && blockIdx.x < g.dbg_max) {}
    __device__ __forceinline__ unsigned long long* slot(int i) const { return on ? dbg + 8L * blockIdx.x + i : nullptr; }
    __device__ __forceinline__ void begin() const {
        if (!on) return;
        unsigned long long* d = slot(0);
        d[0] = __builtin_amdgcn_s_memtime();
        d[4] = __builtin_amdgcn_s_memrealtime();
        d[6] = 0;
        d[5] = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 20) << 32);
    }
    __device__ __forceinline__ void mark(int i) const {
        if (on) *slot(i) = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void end() const {
        if (!on) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *slot(3) = __builtin_amdgcn_s_memtime();
        *slot(6) = __builtin_amdgcn_s_memrealtime();
    }
};

// The plain store of TM accumulators of 32 rows x this lane's column.  Element r of lane half lh is row
// (r & 3) + 8 * (r >> 2) + 4 * lh of its block -- the accumulator layout of v_mfma_f32_32x32x2_f32 and of
// v_mfma_f32_32x32x16_bf16 alike.  c0: the column's element of row 0 (ld: row pitch); bj: its bias (0 without);
// act: 0 none, 1 ReLU, 2 sigmoid; rows from m0 on, below M; tm_eff: row blocks the tile has.
template <int TM>
__device__ __forceinline__ void store_rows(const f32x16* acc, float* c0, long ld, float bj, int act, int m0, int M, int tm_eff, int lh) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (i < tm_eff && row < M) {   // (a 32-row tile owns only its first row block)
                float v = acc[i][r] + bj;
                if (act == 1) v = as_relu(v);
                else if (act == 2) v = as_sigmoid(v);
                c0[(long)row * ld] = v;
            }
        }
}

// ---- the LayerNorm epilogues.  The accumulators of a block of 32 rows (per group of 8 column waves) go to LDS, then every
// wave normalises FOUR rows at a time: lane = (row rr = lane >> 4, slot jj = lane & 15) holds the 16 features
// 64 c + 4 jj + e (c, e < 4) of its row -- four ds_read_b128 that are conflict-free (the 16 lanes one LDS cycle serves read
// 256 consecutive bytes of two rows), row sums by four DPP steps inside the 16-lane row, stores as four
// global_store_dwordx4 of 256 consecutive bytes per row.  (Before: one wave per row, 64 lanes x 4 features, two 64-lane sums
// with v_readlane each and an IEEE 1 / sqrt per row, the four rows of a wave one after the other: 12 k cycles per 64-row
// tile, as long as the split-arithmetic main loop.)
//   NWC  column waves per row block (8).  Waves of row group wm = wave / NWC own tile rows wm * 64 + i * 32 + ...; the
//        staging area holds one 32-row block per row group: [groups * 32][BN] floats.  groups (1 | 2) = row groups that hold
//        rows of the tile; tm_eff = their row blocks (a workgroup may have more waves than that: they only keep the barriers).
//   EPI_LNF: x = relu(acc + bias); C = (x - mean) * rstd; rstd; bits (x > 0, one 32-bit piece per (row, column wave), taken
//            from the accumulators by ballot before they leave for LDS).
//   EPI_LNB: C = relu'(bits_in) * rstd_in * (acc - mean(acc) - xhat * mean(acc * xhat)).
template <int TM, int EPI, int NWC>
__device__ __forceinline__ void lin_ln_rows(const LinK& g, f32x16 (&acc)[TM], float* smem, int bz, int m0, int tm_eff, int groups, int wave,
                                            int lane, float bj) {
    const int l31 = lane & 31, lh = lane >> 5;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wn = wave_u % NWC, wm = wave_u / NWC;       // column wave, row group
    const int col = wn * 32 + l31;
    const int rr = lane >> 4, jj = lane & 15;
    constexpr float inv_d = 1.0f / BN;
    // staged row of this lane in the normalisation phase: 4 * wave + rr of the NG * 32 staged rows; its tile row
    const int srow = 4 * wave_u + rr;
    const int trow_base = (srow >> 5) * 64 + (srow & 31);      // + i * 32
    const bool stages = wm < groups, normalises = 4 * wave_u < 32 * groups;   // (wave-uniform)
    // backward: everything this wave reads from global memory is requested up front (vector memory operations retire in
    // order: a load issued behind the first block's stores would wait for them)
    f32x4 h[TM][4];
    float rs_in[TM];
    u32x4 mw[TM][2];
    if (EPI == EPI_LNB && normalises) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const long row = min((long)m0 + trow_base + i * 32, (long)g.M - 1);
            const float* xr = g.xhat + (long)bz * g.x_batch + row * g.ldx + 4 * jj;
#pragma unroll
            for (int c = 0; c < 4; ++c) h[i][c] = *reinterpret_cast<const f32x4*>(xr + 64 * c);
            rs_in[i] = g.rstd_in[row * g.batch + bz];
            const u32x4* mp = reinterpret_cast<const u32x4*>(g.bits_in + (row * g.batch + bz) * 4);
            mw[i][0] = mp[0];
            mw[i][1] = mp[1];
        }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        if (i >= tm_eff) break;
        if (i > 0) as_lds_barrier();    // the previous block's rows are all read
        float* st = smem + wm * 32 * BN;
        if (!stages) {
        } else if (EPI == EPI_LNF) {
            unsigned mine = 0;        // lane L < 32: the mask piece (columns 32 wn .. 32 wn + 31) of block row L
            // (v_writelane_b32 with the lane as an immediate: one instruction per piece -- a compare + select per piece would be
            // four, and two scalar operands violate the constant-bus limit -- hence a macro over the literal register index)
#define AS_LN_STAGE(r)                                                                                                        \
            {                                                                                                                 \
                const float v = as_relu(acc[i][r] + bj);                                                                      \
                const unsigned long long b = __ballot(v > 0.f);                                                               \
                /* gfx950: a scalar register written by a vector compare needs two wait states before a vector instruction */  \
                /* reads it; hipcc's hazard pass does not look into inline assembly (seen: a stale mask piece, rarely)   */  \
                asm volatile("s_nop 1\n\tv_writelane_b32 %0, %1, %2" : "+v"(mine) : "s"((unsigned)b), "i"(((r) & 3) + 8 * ((r) >> 2))); \
                asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(mine) : "s"((unsigned)(b >> 32)), "i"(((r) & 3) + 8 * ((r) >> 2) + 4)); \
                st[(((r) & 3) + 8 * ((r) >> 2) + 4 * lh) * BN + col] = v;                                                     \
            }
            AS_LN_STAGE(0) AS_LN_STAGE(1) AS_LN_STAGE(2) AS_LN_STAGE(3) AS_LN_STAGE(4) AS_LN_STAGE(5) AS_LN_STAGE(6) AS_LN_STAGE(7)
            AS_LN_STAGE(8) AS_LN_STAGE(9) AS_LN_STAGE(10) AS_LN_STAGE(11) AS_LN_STAGE(12) AS_LN_STAGE(13) AS_LN_STAGE(14) AS_LN_STAGE(15)
#undef AS_LN_STAGE
            const long brow = (long)m0 + wm * 64 + i * 32 + lane;
            if (lane < 32 && brow < g.M) reinterpret_cast<unsigned*>(g.bits)[(brow * g.batch + bz) * 8 + wn] = mine;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[((r & 3) + 8 * (r >> 2) + 4 * lh) * BN + col] = acc[i][r];
        }
        as_lds_barrier();
        if (!normalises) continue;
        const long row = (long)m0 + trow_base + i * 32;
        f32x4 v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = *reinterpret_cast<const f32x4*>(smem + srow * BN + 64 * c + 4 * jj);
        float* o = g.C + (long)bz * g.c_batch + row * g.ldc + 4 * jj;
        if (EPI == EPI_LNF) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
            const float mean = as_row16_sum(s) * inv_d;
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[c] -= mean;
                q += (v[c].x * v[c].x + v[c].y * v[c].y) + (v[c].z * v[c].z + v[c].w * v[c].w);
            }
            const float rs = 1.0f / sqrtf(as_row16_sum(q) * inv_d + g.eps);
            if (row < g.M) {
#pragma unroll
                for (int c = 0; c < 4; ++c) *reinterpret_cast<f32x4*>(o + 64 * c) = v[c] * rs;
                if (jj == 0) g.rstd[row * g.batch + bz] = rs;
            }
        } else {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s1 += (v[c].x + v[c].y) + (v[c].z + v[c].w);
                s2 += (v[c].x * h[i][c].x + v[c].y * h[i][c].y) + (v[c].z * h[i][c].z + v[c].w * h[i][c].w);
            }
            const float m1 = as_row16_sum(s1) * inv_d, m2 = as_row16_sum(s2) * inv_d;
            if (row < g.M) {
                const float rs = rs_in[i];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    // mask word c (64 bits: features 64 c ..): this lane's four bits sit at 4 jj
                    const unsigned lo = c == 0 ? mw[i][0].x : c == 1 ? mw[i][0].z : c == 2 ? mw[i][1].x : mw[i][1].z;
                    const unsigned hi = c == 0 ? mw[i][0].y : c == 1 ? mw[i][0].w : c == 2 ? mw[i][1].y : mw[i][1].w;
                    const unsigned nib = (jj < 8 ? lo : hi) >> (4 * (jj & 7));
                    f32x4 d = (v[c] - m1 - h[i][c] * m2) * rs;
                    d.x = (nib & 1u) ? d.x : 0.f;
                    d.y = (nib & 2u) ? d.y : 0.f;
                    d.z = (nib & 4u) ? d.z : 0.f;
                    d.w = (nib & 8u) ? d.w : 0.f;
                    *reinterpret_cast<f32x4*>(o + 64 * c) = d;
                }
            }
        }
    }
}

// ---- epilogue of the 256-column kernels (8 waves, wave w owns columns 32 w .. 32 w + 31 of all BM rows).
// D[row][col]: col = wave * 32 + l31, row = i * 32 + store_rows' row of r.  `smem`: >= 32 * BN floats, free of readers (behind a barrier).
template <int TM, int EPI>
__device__ __forceinline__ void lin_epilogue(const LinK& g, f32x16 (&acc)[TM], float* smem, int bz, int m0, int tm_eff, int wave, int lane) {
    const int l31 = lane & 31, lh = lane >> 5;
    const int col = wave * 32 + l31;
    if (EPI == EPI_PLAIN) {
        if (col < g.N) {
            const float bj = g.bias ? g.bias[(long)bz * g.bias_batch + col] : 0.f;
            store_rows<TM>(acc, g.C + (long)bz * g.c_batch + col, g.ldc, bj, g.act, m0, g.M, tm_eff, lh);
        }
        return;
    }
    const float bj = (EPI == EPI_LNF && g.bias) ? g.bias[(long)bz * g.bias_batch + col] : 0.f;
    lin_ln_rows<TM, EPI, 8>(g, acc, smem, bz, m0, tm_eff, 1, wave, lane, bj);
}

// NBUF ring slots: two k-tiles in flight, 60 KB: two workgroups per CU
template <int BM, bool B_KC, int EPI>
__global__ __launch_bounds__(NT, 4) void lin_f32_kernel(LinK g) {
    constexpr int TM = BM / 32;
    constexpr int TILE = BK * (BM + BN);
    constexpr int PA_TOTAL = BM / 16;    // 1-KiB DMA pieces of the A tile (16 rows x 16 k each)
    constexpr int RING = NBUF * TILE, EPIT = 32 * BN;
    constexpr int AHEADT = NBUF - 1;     // k-tiles in flight besides the one being multiplied
    __shared__ __attribute__((aligned(16))) float smem[RING > EPIT ? RING : EPIT];

    static_assert(BM == 64, "tile_of: tiles of 64 and of 32 rows");
    const Tile t = tile_of<false>(g);
    const int bz = t.bz, m0 = t.m0, tm_eff = t.tm;
    const float* __restrict__ A = g.A + (long)bz * g.a_batch;
    const float* __restrict__ B = g.B + (long)bz * g.b_batch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;

    // ---- DMA sources (per lane) and destinations (per wave)
    // A: piece p = rows 16p .. 16p+15 of the tile; lane -> row 16p + (lane >> 2), LDS chunk slot lane & 3, which receives the
    // global chunk slot ^ ((row >> 2) & 3).  Every wave issues ONE A piece: waves 4-7 re-issue pieces 0-3 (identical bytes to
    // identical addresses) so that all waves count the same number of DMAs per k-tile.
    // Chunks at or beyond ka_valid (a reduction padded up to a multiple of 16 whose B rows there are zero) re-read chunk 0.
    const int pa = wave % PA_TOTAL;
    const int ra = pa * 16 + (lane >> 2);
    const int a_gc = ((lane & 3) ^ ((ra >> 2) & 3)) * 4;
    const float* a_src = A + (long)min(m0 + ra, g.M - 1) * g.lda + a_gc;
    // B: 16 pieces, two per wave.  B_KC: piece = 16 rows (output features) x 16 k, swizzled like A.  Else: piece = one k row
    // of 256 output features.
    const float* b_src[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = wave * 2 + j;
        if (B_KC) {
            const int r = p * 16 + (lane >> 2);
            const int gc = (lane & 3) ^ ((r >> 2) & 3);
            b_src[j] = B + (long)min(r, g.N - 1) * g.ldb + gc * 4;
        } else {
            b_src[j] = B + (long)p * g.ldb + min(lane * 4, g.N - 4);
        }
    }
    const unsigned smem_base = as_lds_addr(smem);
    // piece 0 = this wave's A piece, pieces 1, 2 = its two B pieces of k-tile kt
    auto issue_piece = [&](int kt, int piece) {
        const unsigned base = smem_base + (unsigned)((kt % NBUF) * TILE) * 4u;
        const int k0 = kt * BK;
        if (piece == 0) {
            const bool ok = k0 + a_gc + 4 <= g.ka_valid;
            as_glds16(a_src + (ok ? k0 : -a_gc), base + (unsigned)(pa * 1024));
        } else {
            const int j = piece - 1;
            as_glds16(b_src[j] + (B_KC ? (long)k0 : (long)k0 * g.ldb), base + (unsigned)((BK * BM + (wave * 2 + j) * 256) * 4));
        }
    };
    auto issue = [&](int kt) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) issue_piece(kt, pc);
    };

    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    const int nk = g.K / BK;
    const Stamps stamps(g, tid);
    stamps.begin();
    const int swz = (l31 >> 2) & 3;   // rows i * 32 + l31 and wave * 32 + l31 share it (32 = 0 mod 16)
    // two k-tiles in flight; the older one is retired with vmcnt(3).  (A 2-slot ring with three workgroups per CU was no
    // faster: 108-118 us against 108-114 for head GEMM 2.)
    issue(0);
    if (nk > 1) issue(1);
    if (nk > 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    stamps.mark(1);
    // Main loop, software-pipelined across the k-tile boundary.  A k-tile is two 8-deep fragment groups; the barrier that
    // ends a tile sits BETWEEN the two groups' MFMAs: when a wave reaches it, all its LDS reads of the tile are in registers
    // and eight MFMAs are still to be issued, and right behind it the first fragments of the NEXT tile are requested, so
    // the barrier's skew and the LDS round trip run under matrix work instead of in front of it (before: every tile began
    // with all eight waves waiting for their first fragments, ~10 % of a 2048-cycle tile with the pipe idle).
    struct Frag { float4 av[TM]; float bv[4]; };
    auto load = [&](Frag& f, int kt_, int cc) {
        const float* tile = smem + (kt_ % NBUF) * TILE;
        const float* a_s = tile + l31 * BK;
        const float* b_s = tile + BK * BM;
        const int slot = ((2 * cc + lh) ^ swz) * 4;
#pragma unroll
        for (int i = 0; i < TM; ++i) f.av[i] = *reinterpret_cast<const float4*>(a_s + i * 32 * BK + slot);
        if (B_KC) {
            const float4 t = *reinterpret_cast<const float4*>(b_s + (wave * 32 + l31) * BK + slot);
            f.bv[0] = t.x; f.bv[1] = t.y; f.bv[2] = t.z; f.bv[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) f.bv[j] = b_s[(cc * 8 + 4 * lh + j) * BN + wave * 32 + l31];
        }
    };
    // dma_kt >= 0: the three DMA pieces of k-tile dma_kt are issued BETWEEN the MFMAs (one after each of the first three
    // k-steps): an LDS-DMA costs the issuing wave ~60-180 cycles of instruction issue, and as a block at the top of the tile
    // -- every wave of the workgroup at the same moment, right behind the barrier -- those cycles were matrix-pipe idle
    // time; behind an MFMA they run while the pipe works on it.
    auto mma = [&](const Frag& f, int dma_kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if (i < tm_eff) {   // (a 32-row tile owns only its first row block)
                    const float a = j == 0 ? f.av[i].x : j == 1 ? f.av[i].y : j == 2 ? f.av[i].z : f.av[i].w;
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, f.bv[j], acc[i], 0, 0, 0);
                }
            }
            if (j < 3 && dma_kt >= 0) {
                __builtin_amdgcn_sched_barrier(0);
                issue_piece(dma_kt, j);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    static_assert(BK == 16, "two fragment groups per k-tile");
    Frag f0, f1;
    load(f0, 0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        load(f1, kt, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(f0, kt + AHEADT < nk ? kt + AHEADT : -1);
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        as_wait_lds();     // this wave's reads of slot kt % NBUF are in registers
        __builtin_amdgcn_s_barrier();
        if (kt + 1 < nk) load(f0, kt + 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        mma(f1, -1);
        __builtin_amdgcn_sched_barrier(0);
    }
    stamps.mark(2);

    lin_epilogue<TM, EPI>(g, acc, smem, bz, m0, tm_eff, wave, lane);
    stamps.end();
}

// ---------------------------------------------------------------------------------------------------------------------
// The same layers with the products on the bfloat16 matrix instruction (v_mfma_f32_32x32x16_bf16: 16 x the rate of
// v_mfma_f32_32x32x2_f32), fp32 in, fp32 out, fp32 accumulation.  An fp32 number is EXACTLY the sum of three bfloat16
// numbers (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): 8 + 8 + 8 significand bits), so a product a.b is the
// sum of nine plane products with exact operands; the three smallest (lo.lo, lo.mid, mid.lo, each <= 2^-24 |a||b|) are
// dropped: six MFMAs per 16-deep k-step.  Against an fp64 product of the same fp32 operands this is MORE accurate than the
// fp32 matrix instruction (rms 2.4e-7 vs 2.9e-7 of rms C: the bf16 instruction adds 16 products before it rounds, the fp32
// one two; profiles/r03_split_gemm_probe.log, tests/test_gpu_parity.py::test_split_matrix_arithmetic_*).
//   * B (the folded weights) arrives as planes, emitted once per step by as_emit_planes (rowops.hip) k-step-major:
//     [plane][head][K / 16][rows][16] bf16, so that the fragment of a wave (32 columns x 8 k x 2 lane halves) is 1 KiB of
//     consecutive bytes.  A wave's columns are its own: B fragments go from L2 straight to registers (global_load_dwordx4,
//     two k-steps ahead in three name-rotated register sets), not through the LDS.
//   * A (activations / gradients) stays fp32 in HBM.  Each thread loads 4 consecutive k of one row per 32-deep k-tile (two
//     tiles ahead), splits them (v_cvt_pk_bf16_f32 + v_pk_add_f32: 4.5 vector instructions per element, once per workgroup)
//     and writes 3 x 8 bytes into the plane image of the tile in LDS ([plane][64 rows][32 k] bf16 = 64-byte rows, the four
//     16-byte chunks of a row XOR-swizzled by (row >> 2) & 3: the 16 lanes a ds_read_b128 serves per LDS cycle -- rows
//     {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} -- then touch each of the 64 banks once).  All eight
//     waves read their A fragments from there: one barrier per 32-deep k-tile, two plane images (24 KB).
//   * accumulator layout = that of the fp32 instruction: the LayerNorm epilogues above are shared.

constexpr int S6_BK = 32;                 // k-tile of the A image (two MFMA k-steps)
constexpr int S6_PLANE = 64 * S6_BK * 2;  // bytes of one plane of one k-tile: 64 rows x 32 bf16
constexpr int S6_BUF = 3 * S6_PLANE;

// The main loop shared by the 256-column kernel (NW = 8 waves) and the output layer's (NW = 4): 64 rows x 32 NW columns,
// wave w = columns 32 w .. 32 w + 31 of all 64 rows (two accumulators).  `sm`: 2 x S6_BUF bytes.
//   A / lda: first row of the tile's operand rows (row index clamped to rows_valid - 1), k >= ka_valid reads as zero
//   bp (wave-uniform) + b_lane bytes: this lane's B fragment of plane 0, k-step 0; plane stride bp_plane, k-step stride bp_step (elements)
//   (rows of A within 2^31 bytes of the tile's first: lda < 2^23 floats)
template <int NW, int TME>   // TME: row blocks of 32 the tile really has (a 32-row tile multiplies only the first)
__device__ __forceinline__ void s6_main_loop(f32x16 (&acc)[2], unsigned char* sm, const float* __restrict__ A, long lda, int rows_valid,
                                             int K, int ka_valid, const uint16_t* __restrict__ bp, unsigned b_lane, long bp_plane,
                                             long bp_step, int tid, int lane, bool late, unsigned long long* stamp1 = nullptr) {
    constexpr int NTH = NW * 64;
    constexpr int AL = 512 / NTH;         // float4 loads per thread and k-tile (64 rows x 8 chunks of 4 k)
    const int l31 = lane & 31, lh = lane >> 5;
    const int a_chunk = tid & 7;
    // every global access = wave-uniform base pointer + 32-bit lane offset (the scalar-base form of global_load: no 64-bit
    // vector address arithmetic, no address register pairs)
    unsigned a_off[AL];
    int a_wr[AL];
#pragma unroll
    for (int q = 0; q < AL; ++q) {
        const int row = (tid >> 3) + q * (NTH / 8);
        a_off[q] = (unsigned)(min(row, rows_valid - 1) * (int)lda + a_chunk * 4) * 4u;   // bytes
        a_wr[q] = row * 64 + (((a_chunk >> 1) ^ ((row >> 2) & 3)) * 16) + (a_chunk & 1) * 8;
    }
    const int nk = K / S6_BK, nj = 2 * nk;
    const gptr Au = as_uniform_ptr(A);
    // every load below is unconditional (indices clamped to the last tile / k-step): straight-line code, so that hipcc's
    // s_waitcnt vmcnt counts are exact -- a load under a branch makes every later wait assume the branch was not taken,
    // i.e. wait for (nearly) everything in flight
    auto a_load = [&](f32x4 (&dst)[AL], int kt) {
        kt = min(kt, nk - 1);
        // chunks at or beyond ka_valid (a reduction padded up to the tile whose B rows there are zero planes) re-read chunk 0
        // of the row: an ADDRESS select -- a value select would put the load itself under a branch
        // (the offset stays non-negative: it is zero-extended by the scalar-base form)
        const unsigned ko = kt * S6_BK + a_chunk * 4 + 4 <= ka_valid ? (unsigned)(kt * S6_BK) * 4u : 0u - (unsigned)a_chunk * 16u;
#pragma unroll
        for (int q = 0; q < AL; ++q) dst[q] = *reinterpret_cast<gptr_f4>(Au + (a_off[q] + ko));
    };
    auto a_store = [&](const f32x4 (&src)[AL], int buf) {
#pragma unroll
        for (int q = 0; q < AL; ++q) {
            unsigned h0, m0, l0, h1, m1, l1;
            split_pair(src[q].x, src[q].y, h0, m0, l0);
            split_pair(src[q].z, src[q].w, h1, m1, l1);
            unsigned char* d = sm + buf * S6_BUF + a_wr[q];
            *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(d + S6_PLANE) = make_uint2(m0, m1);
            *reinterpret_cast<uint2*>(d + 2 * S6_PLANE) = make_uint2(l0, l1);
        }
    };
    auto b_load = [&](u32x4 (&dst)[3], int j) {
        j = min(j, nj - 1);
#pragma unroll
        for (int p = 0; p < 3; ++p) dst[p] = *reinterpret_cast<gptr_u4>(as_uniform_ptr(bp + p * bp_plane + j * bp_step) + b_lane);
    };
    int sw = (l31 >> 2) & 3;              // rows i * 32 + l31 share it (32 = 0 mod 16)
    const unsigned char* a_rd = sm + l31 * 64;
    int lh_rd = lh;                       // (sw, a_rd, lh_rd: recomputed behind the loop for the tail tiles, see there)

    f32x4 aq[3][AL];
    u32x4 bq[3][3];
    a_load(aq[0], 0);
    a_load(aq[1], 1);
    b_load(bq[0], 0);
    b_load(bq[1], 1);
    a_store(aq[0], 0);
    as_lds_barrier();
    if (stamp1) *stamp1 = __builtin_amdgcn_s_memtime();
    // k-tile kt (kt % 3 == U): its plane image is in buffer kt & 1, its B fragments in sets (2 kt) % 3 and (2 kt + 1) % 3
    auto tile = [&](auto Uc, int kt) {
        constexpr int U = decltype(Uc)::value;
        const unsigned char* img = a_rd + (kt & 1) * S6_BUF;
        a_load(aq[(U + 2) % 3], kt + 2);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            b_load(bq[(2 * U + s + 2) % 3], 2 * kt + s + 2);
            __builtin_amdgcn_sched_barrier(0);   // the look-ahead loads stay HERE, two k-steps in front of their first use
            bf16x8 fa[TME][3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int i = 0; i < TME; ++i)
                    fa[i][p] = *reinterpret_cast<const bf16x8*>(img + p * S6_PLANE + i * 32 * 64 + (((2 * s + lh_rd) ^ sw) * 16));
            const u32x4(&bs)[3] = bq[(2 * U + s) % 3];
            bf16x8 fb[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) fb[p] = __builtin_bit_cast(bf16x8, bs[p]);
            // six of the nine plane products (without mid.lo, lo.mid, lo.lo).  Those with the hi plane of A first: the first six
            // MFMAs need two of the six LDS reads, the mid / lo fragments arrive under them.  (The order does not matter to the
            // result's error: the accumulator already holds the sum of the earlier k-steps.)
            constexpr int PA[6] = {0, 0, 0, 1, 1, 2}, PB[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
            for (int o = 0; o < 6; ++o)
#pragma unroll
                for (int i = 0; i < TME; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][PA[o]], fb[PB[o]], acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            // The split of the NEXT tile (vector + LDS-store work, no matrix work) sits at a different place in the two halves of
            // the workgroup: waves 0-3 behind the tile's second k-step, waves 4-7 between the two.  Waves w and w + 4 share a
            // SIMD and, running the same program between the same barriers, would otherwise do their vector work at the same
            // moment and their matrix work at the same moment -- the matrix pipe idles through the former.
            if (late == (s == 0)) a_store(aq[(U + 1) % 3], (kt & 1) ^ 1);   // (behind the last tile: a clamped repeat)
        }
        as_lds_barrier();
    };
    int kt = 0;
    for (; kt + 3 <= nk; kt += 3) {
        tile(IC<0>{}, kt);
        tile(IC<1>{}, kt + 1);
        tile(IC<2>{}, kt + 2);
    }
    // The tail tiles address their fragments from a lane index the compiler cannot trace back to the one in front of the loop.
    // Otherwise it keeps the loop's lane-constant fragment offsets (precomputed per k-step) AND the values the tail tiles derive
    // theirs from alive across the loop; in the kernels that are at their register limit those are spilled, and a reload from
    // scratch is a vector-memory operation whose wait (vmcnt(0): operations retire in order) drains the look-ahead loads.
    {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        lh_rd = ln >> 5;
        sw = ((ln & 31) >> 2) & 3;
        a_rd = sm + (ln & 31) * 64;
    }
    if (kt < nk) tile(IC<0>{}, kt);
    if (kt + 1 < nk) tile(IC<1>{}, kt + 1);
}

// A split-arithmetic kernel's way into the main loop for its tile: zeroed accumulators, the tile's rows of A and its head's planes
// from k0 on (klen deep, kav of them valid in A: lin_s6_plain_kernel's chunk of K, everywhere else 0 / K / ka_valid), this lane's
// B fragment, the second half of the waves splitting late, and the 64- or the 32-row loop.
template <int NW, typename K>
__device__ __forceinline__ void s6_tile(const K& g, const Tile& t, f32x16 (&acc)[2], unsigned char* sm, int k0, int klen, int kav, int tid,
                                        unsigned long long* stamp1 = nullptr) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const long bp_step = (long)g.bp_rows * 16;
    const uint16_t* bp = g.Bp + (long)t.bz * g.bp_batch + (k0 / 16) * bp_step;
    const unsigned b_lane = (unsigned)((wave * 32 + (lane & 31)) * 16 + (lane >> 5) * 8) * 2u;   // bytes
    const float* A = g.A + (long)t.bz * g.a_batch + (long)t.m0 * g.lda + k0;
    const bool late = __builtin_amdgcn_readfirstlane(wave) >= NW / 2;
    if (t.tm == 2) s6_main_loop<NW, 2>(acc, sm, A, g.lda, g.M - t.m0, klen, kav, bp, b_lane, g.bp_plane, bp_step, tid, lane, late, stamp1);
    else s6_main_loop<NW, 1>(acc, sm, A, g.lda, g.M - t.m0, klen, kav, bp, b_lane, g.bp_plane, bp_step, tid, lane, late, stamp1);
}

template <int EPI>
__global__ __launch_bounds__(NT, 4) void lin_s6_kernel(LinK g) {
    constexpr int EPIT = 32 * BN;
    static_assert(EPIT * 4 >= 2 * S6_BUF, "the epilogue's staging area holds both plane images");
    __shared__ __attribute__((aligned(16))) float smem[EPIT];
    const Tile t = tile_of<true>(g);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Stamps stamps(g, tid);
    stamps.begin();
    f32x16 acc[2];
    s6_tile<8>(g, t, acc, reinterpret_cast<unsigned char*>(smem), 0, g.K, g.ka_valid, tid, stamps.slot(1));
    stamps.mark(2);
    lin_epilogue<2, EPI>(g, acc, smem, t.bz, t.m0, t.tm, wave, lane);
    stamps.end();
}

// ---------------------------------------------------------------------------------------------------------------------
// Short reductions (K <= S6R_MAXK = 128: Linear 1 at H <= 128, dx3): the plane image of the tile's WHOLE A operand fits in
// LDS at once ([nk][plane][64 rows][32 k] bf16: nk x S6_BUF <= 48 KB), so the k-loop needs neither the A pipeline nor its
// barriers.  s6_main_loop is built for long reductions -- per 32-deep k-tile an A load two tiles ahead, a split, an LDS store
// and a barrier -- at four k-tiles four barriers and four load-to-fragment chains for 6.1 k cycles of matrix instructions
// (loop 14.6 k cycles per workgroup, here 10.3 k; what that is worth in time: DESIGN 5, "Short reductions" -- the two tenants
// of a CU meet in their epilogues, and most of Linear 1's gain is the image it shares).  Here every thread requests its A values of
// all k-tiles up front, splits them into the image, ONE barrier follows, and the 2 nk k-steps run with the B look-ahead, the
// fragment reads and the MFMAs only.  Every accumulator sees the sequence it sees in s6_main_loop (k-steps ascending, the six
// plane products in the same order): the results are bit-identical.  8-wave workgroups (one float4 per thread and k-tile).
constexpr int S6R_MAXK = 128, S6R_MAXT = S6R_MAXK / S6_BK;

// This thread's A values of all k-tiles (s6_main_loop's a_load for every tile at once: row clamped to rows_valid - 1, tiles
// beyond nk repeat the last one, chunks at or beyond ka_valid re-read chunk 0 of the row) ...
__device__ __forceinline__ void s6r_image_load(f32x4 (&aq)[S6R_MAXT], const float* __restrict__ A, long lda, int rows_valid, int nk, int ka_valid,
                                               int tid) {
    const int a_chunk = tid & 7, row = tid >> 3;
    const unsigned a_off = (unsigned)(min(row, rows_valid - 1) * (int)lda + a_chunk * 4) * 4u;   // bytes
    const gptr Au = as_uniform_ptr(A);
#pragma unroll
    for (int q = 0; q < S6R_MAXT; ++q) {
        const int kt = min(q, nk - 1);
        const unsigned ko = kt * S6_BK + a_chunk * 4 + 4 <= ka_valid ? (unsigned)(kt * S6_BK) * 4u : 0u - (unsigned)a_chunk * 16u;
        aq[q] = *reinterpret_cast<gptr_f4>(Au + (a_off + ko));
    }
}
// ... and their planes into the image (s6_main_loop's a_store; a repeated tile writes the same bytes to the same place)
__device__ __forceinline__ void s6r_image_store(const f32x4 (&aq)[S6R_MAXT], unsigned char* sm, int nk, int tid) {
    const int a_chunk = tid & 7, row = tid >> 3;
    const int a_wr = row * 64 + (((a_chunk >> 1) ^ ((row >> 2) & 3)) * 16) + (a_chunk & 1) * 8;
#pragma unroll
    for (int q = 0; q < S6R_MAXT; ++q) {
        unsigned h0, m0, l0, h1, m1, l1;
        split_pair(aq[q].x, aq[q].y, h0, m0, l0);
        split_pair(aq[q].z, aq[q].w, h1, m1, l1);
        unsigned char* d = sm + min(q, nk - 1) * S6_BUF + a_wr;
        *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(d + S6_PLANE) = make_uint2(m0, m1);
        *reinterpret_cast<uint2*>(d + 2 * S6_PLANE) = make_uint2(l0, l1);
    }
}

// The B fragments of one head as the loops address them (s6_tile's arguments) and the load of k-step j into a register set
struct S6B { const uint16_t* bp; long bp_plane, bp_step; unsigned b_lane; int nj; };
template <typename K>
__device__ __forceinline__ S6B s6_b_of(const K& g, int bz, int nk, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    S6B b;
    b.bp_step = (long)g.bp_rows * 16;
    b.bp = g.Bp + (long)bz * g.bp_batch;
    b.bp_plane = g.bp_plane;
    b.b_lane = (unsigned)((wave * 32 + (lane & 31)) * 16 + (lane >> 5) * 8) * 2u;   // bytes
    b.nj = 2 * nk;
    return b;
}
__device__ __forceinline__ void s6_b_load(u32x4 (&dst)[3], const S6B& b, int j) {
    j = min(j, b.nj - 1);
#pragma unroll
    for (int p = 0; p < 3; ++p) dst[p] = *reinterpret_cast<gptr_u4>(as_uniform_ptr(b.bp + p * b.bp_plane + j * b.bp_step) + b.b_lane);
}

// The k-steps over a resident image (complete behind a barrier).  bq[0], bq[1]: k-steps 0 and 1 of B, requested by the caller
// (in front of the image's split, or of the previous head's epilogue); the look-ahead stays two k-steps in three name-rotated
// register sets as in s6_main_loop, and so does the tail tiles' opaque lane index.
template <int TME>
__device__ __forceinline__ void s6_resident_loop(f32x16 (&acc)[2], const unsigned char* sm, int nk, const S6B& b, u32x4 (&bq)[3][3], int lane) {
    const int l31 = lane & 31;
    int sw = (l31 >> 2) & 3;
    const unsigned char* a_rd = sm + l31 * 64;
    int lh_rd = lane >> 5;
    auto tile = [&](auto Uc, int kt) {
        constexpr int U = decltype(Uc)::value;
        const unsigned char* img = a_rd + kt * S6_BUF;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            s6_b_load(bq[(2 * U + s + 2) % 3], b, 2 * kt + s + 2);
            __builtin_amdgcn_sched_barrier(0);   // the look-ahead loads stay HERE, two k-steps in front of their first use
            bf16x8 fa[TME][3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int i = 0; i < TME; ++i)
                    fa[i][p] = *reinterpret_cast<const bf16x8*>(img + p * S6_PLANE + i * 32 * 64 + (((2 * s + lh_rd) ^ sw) * 16));
            const u32x4(&bs)[3] = bq[(2 * U + s) % 3];
            bf16x8 fb[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) fb[p] = __builtin_bit_cast(bf16x8, bs[p]);
            constexpr int PA[6] = {0, 0, 0, 1, 1, 2}, PB[6] = {0, 1, 2, 0, 1, 0};   // s6_main_loop's order
#pragma unroll
            for (int o = 0; o < 6; ++o)
#pragma unroll
                for (int i = 0; i < TME; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][PA[o]], fb[PB[o]], acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    int kt = 0;
    if (nk >= 3) {
        tile(IC<0>{}, 0);
        tile(IC<1>{}, 1);
        tile(IC<2>{}, 2);
        kt = 3;
    }
    {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        lh_rd = ln >> 5;
        sw = ((ln & 31) >> 2) & 3;
        a_rd = sm + (ln & 31) * 64;
    }
    if (kt < nk) tile(IC<0>{}, kt);
    if (kt + 1 < nk) tile(IC<1>{}, kt + 1);
}
__device__ __forceinline__ void s6_zero(f32x16 (&acc)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}

// Linear 1 (EPI_LNF, every head reads the same x_hat: a_batch == 0) from ONE image per row tile: a workgroup owns a row tile
// and group t.bz of g.groups groups of consecutive heads (the tile list counts groups where lin_s6_kernel's counts heads),
// builds the image once and runs, head after head, the resident loop on that head's planes and lin_ln_rows into that head's
// C, rstd and bits.  The next head's first two B fragments are requested in front of the epilogue.  The image lives across
// the heads, so the epilogue's 32 KB staging area lies BEHIND it: nk x 12 + 32 KB of dynamic LDS (80 KB at K = 128: two
// workgroups take the CU's whole 160 KB).
__global__ __launch_bounds__(NT, 4) void lin_s6_lnf_shared_kernel(LinK g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    const Tile t = tile_of<true>(g);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Stamps stamps(g, tid);
    stamps.begin();
    const int nk = g.K / S6_BK;
    float* stage = reinterpret_cast<float*>(dsm + nk * S6_BUF);
    const int h0 = t.bz * g.batch / g.groups, h1 = (t.bz + 1) * g.batch / g.groups;
    f32x4 aq[S6R_MAXT];
    u32x4 bq[3][3];
    s6r_image_load(aq, g.A + (long)t.m0 * g.lda, g.lda, g.M - t.m0, nk, g.ka_valid, tid);
    S6B b = s6_b_of(g, h0, nk, tid);
    s6_b_load(bq[0], b, 0);
    s6_b_load(bq[1], b, 1);
    s6r_image_store(aq, dsm, nk, tid);
    as_lds_barrier();
    stamps.mark(1);
    const int col = wave * 32 + (lane & 31);
    for (int h = h0; h < h1; ++h) {
        f32x16 acc[2];
        s6_zero(acc);
        if (t.tm == 2) s6_resident_loop<2>(acc, dsm, nk, b, bq, lane);
        else s6_resident_loop<1>(acc, dsm, nk, b, bq, lane);
        b = s6_b_of(g, min(h + 1, h1 - 1), nk, tid);   // (behind the last head: a repeat)
        s6_b_load(bq[0], b, 0);
        s6_b_load(bq[1], b, 1);
        const float bj = g.bias ? g.bias[(long)h * g.bias_batch + col] : 0.f;
        if (h > h0) as_lds_barrier();    // the previous head's staged rows are all read
        lin_ln_rows<2, EPI_LNF, 8>(g, acc, stage, h, t.m0, t.tm, 1, wave, lane, bj);
    }
    stamps.mark(2);                      // (slot 2 - slot 1: every head's loop and epilogue)
    stamps.end();
}

// dx3 (EPI_LNB at Npad <= 128) on the resident loop: one head per workgroup as in lin_s6_kernel; the image is dead behind the
// loop, so the epilogue's staging area lies over it: 48 KB, two workgroups per CU.
__global__ __launch_bounds__(NT, 4) void lin_s6_lnb_short_kernel(LinK g) {
    constexpr int EPIT = 32 * BN;
    __shared__ __attribute__((aligned(16))) unsigned char sm[S6R_MAXT * S6_BUF];
    static_assert(S6R_MAXT * S6_BUF >= EPIT * 4, "the image's memory holds the epilogue's staging area");
    const Tile t = tile_of<true>(g);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Stamps stamps(g, tid);
    stamps.begin();
    const int nk = g.K / S6_BK;
    f32x4 aq[S6R_MAXT];
    u32x4 bq[3][3];
    s6r_image_load(aq, g.A + (long)t.bz * g.a_batch + (long)t.m0 * g.lda, g.lda, g.M - t.m0, nk, g.ka_valid, tid);
    const S6B b = s6_b_of(g, t.bz, nk, tid);
    s6_b_load(bq[0], b, 0);
    s6_b_load(bq[1], b, 1);
    s6r_image_store(aq, sm, nk, tid);
    as_lds_barrier();
    stamps.mark(1);
    f32x16 acc[2];
    s6_zero(acc);
    if (t.tm == 2) s6_resident_loop<2>(acc, sm, nk, b, bq, lane);
    else s6_resident_loop<1>(acc, sm, nk, b, bq, lane);
    stamps.mark(2);
    as_lds_barrier();                    // every wave's fragments are in registers: the staging area may overwrite the image
    lin_ln_rows<2, EPI_LNB, 8>(g, acc, reinterpret_cast<float*>(sm), t.bz, t.m0, t.tm, 1, wave, lane, 0.f);
    stamps.end();
}

// A plain Linear on the same main loop: C = act(A . B^T + bias), 64 (or 32) rows x 32 NW columns per workgroup (NW = 8:
// N <= 256, NW = 4: N <= 128; four workgroups per CU at NW = 4), optionally split over K (gridDim.y chunks of kchunk, each
// writing its partial sums -- no bias, no activation -- to its own slab C + y * c_split: the consumer adds them in a fixed order).
// WPS = waves per SIMD the kernel is compiled for.  At 4 (128 VGPRs) the 64-row loop of NW = 4 does not fit (it needs 137: two
// A loads per thread and k-tile), and what does not fit is reloaded from scratch INSIDE the loop -- a vector-memory operation,
// whose wait (vmcnt(0), operations retire in order) drains every look-ahead load of s6_main_loop.  A launch that never has four
// workgroups of a CU resident (the heads' dx1: two at most) takes WPS = 2, which compiles without scratch.
template <int NW, int WPS>
__global__ __launch_bounds__(NW * 64, WPS) void lin_s6_plain_kernel(LinK g) {
    __shared__ __attribute__((aligned(16))) unsigned char sm[2 * S6_BUF];
    const Tile t = tile_of<true>(g);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ks = blockIdx.y, k0 = ks * g.kchunk;
    const int klen = min(g.kchunk, g.K - k0);
    f32x16 acc[2];
    s6_tile<NW>(g, t, acc, sm, k0, klen, max(0, min(klen, g.ka_valid - k0)), tid);
    const int col = wave * 32 + (lane & 31);
    if (col >= g.N) return;
    const bool whole = gridDim.y == 1;
    const float bj = (whole && g.bias) ? g.bias[(long)t.bz * g.bias_batch + col] : 0.f;
    store_rows<2>(acc, g.C + (long)ks * g.c_split + (long)t.bz * g.c_batch + col, g.ldc, bj, whole ? g.act : 0, t.m0, g.M, t.tm, lane >> 5);
}

// ---------------------------------------------------------------------------------------------------------------------
// Output layer of the heads: out = sigmoid(x_hat . W3'^T + b3') (models.py:28-31, 145), N = 2 x n_samples <= 128 columns per
// head, optionally with the training criterion fused into the epilogue (EuclideanDistance + padding mask + mean,
// phoneme_to_articulation/metrics.py:17-24, train_phoneme_to_articulation.py:86-90, and its gradient through the sigmoid).
// One workgroup = 64 frames x the (<= 128) outputs of ONE head: 2 x 4 waves, a wave owns 32 rows x 32 columns (one
// accumulator), so none of the eight waves multiplies padding beyond the N -> 128 round-up (the 256-column kernel above would
// leave four of its eight waves on zeros).  36 KB of LDS, < 64 VGPRs: four workgroups per CU.  Same LDS-DMA ring as above
// (16-deep k-tiles, XOR-swizzled 16-byte chunks, counted vmcnt, raw barriers); every wave issues one A piece (waves 4-7
// repeat pieces 0-3) and one B piece per k-tile.
// Fused criterion: the x coordinates (columns [0, N/2)) and y coordinates ([N/2, N)) of a point lie in different waves, so
// the sigmoid outputs of the tile meet in LDS (the ring's memory); a thread then owns (frame, point) pairs: distance to the
// target, its share of the masked sum, and d loss / d(pre-sigmoid) written where the backward expects d(out).  Partial sums
// leave per workgroup and are added in a fixed order by loss_final (deterministic).
constexpr int ON = 128;

struct LinOutK {
    const float* A; long lda, a_batch;       // x_hat [M][batch][K]
    const float* B; long ldb, b_batch; int b_rows;   // W3' [batch][b_rows >= N][K] (rows N .. b_rows-1 zero)
    const float* bias; long bias_batch;
    float* out; long ldo, o_batch;           // [M][batch][N]
    int M, N, K, batch;
    int n_big, big_per_batch, big_per_batch_rows, small_per_batch;
    // fused criterion (tgt == nullptr: plain output layer)
    const float* tgt; long tgt_T; const int* lengths; int T; float scale;
    float* dout; float* partial;
    const uint16_t* Bp; long bp_plane, bp_batch; int bp_rows;   // lin_out_s6_kernel: W3' as bfloat16 planes (as_lin_out.Bp)
    float* loss; int* counter;                                  // the last workgroup sums the partials (as_lin_out.loss)
    int row_epi;                                                // fused criterion through criterion_rows_f4 (as_lin_out_try decides)
};

// The criterion's workgroup sum goes out; with an arrival counter the workgroup that delivers the last one adds them all, thread
// i taking partials i, i + 256, ... and the 256 sums meeting as in loss_final_kernel (metrics.hip): the same value, bit for bit.
// Partials are written through to memory and read back at agent scope (another XCD's L2 does not see a plain store: gemm_f32.hip).
__device__ __forceinline__ void criterion_tail(const LinOutK& g, int tile, float sum, int tid, float* red) {
    if (g.counter == nullptr) {
        if (tid == 0) g.partial[tile] = sum;
        return;
    }
    __shared__ int s_last;
    if (tid == 0) {
        __hip_atomic_store(&g.partial[tile], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int last = atomicAdd(g.counter, 1) == (int)gridDim.x - 1;
        if (last) __hip_atomic_store(g.counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    float s = 0.f;
    if (tid < 256)
        for (int i = tid; i < (int)gridDim.x; i += 256) s += __hip_atomic_load(&g.partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s = as_wave_sum(s);
    __syncthreads();                 // `red` held the workgroup's own wave sums until here
    if ((tid & 63) == 0 && tid < 256) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) g.loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) * g.scale;
}

// The fused criterion of a workgroup of NW waves, from the tile's sigmoid outputs in LDS (`tile`: [64][ON], complete behind a
// barrier) on: out, d loss / d(pre-sigmoid), and the workgroup's share of the masked sum.  One wave per frame (row) at a time,
// lanes over the points: frame index, utterance, validity and the target row are wave-uniform (computed once per row on the
// scalar unit, no per-pair divisions).  A lane owns ONE point of each of the wave's 64 / NW frames: N <= ON outputs are at most
// 64 points.  ALL target coordinates are requested before the first store goes out: vector memory operations retire in
// order, so a target load issued behind a frame's stores waits for their acknowledgement -- frame after frame, that chain was
// most of this epilogue (and two passes of 8 frames cost the second pass of lin_out_s6_kernel exactly that).
static_assert(ON / 2 <= 64, "criterion_rows: a lane owns one point of a frame");

// One point of a frame: its distance added to `part`, d loss / d(pre-sigmoid) to gx, gy (zeros for a padded frame).  Written
// once: criterion_rows and criterion_rows_f4 must round alike.
__device__ __forceinline__ void criterion_point(float ox, float oy, float tx, float ty, bool valid, float scale, float& part, float& gx, float& gy) {
    gx = 0.f;
    gy = 0.f;
    if (valid) {
        const float dx = ox - tx, dy = oy - ty;
        const float d = sqrtf(dx * dx + dy * dy);
        part += d;
        const float gg = scale / d;                     // NaN at zero distance, as torch autograd
        gx = dx * gg * ox * (1.f - ox);                  // through the sigmoid (same product order as the unfused kernels)
        gy = dy * gg * oy * (1.f - oy);
    }
}

// The lanes' sums of a workgroup of NW waves -> one partial per tile (criterion_tail).
template <int NW>
__device__ __forceinline__ void criterion_sum(const LinOutK& g, float part, int tid) {
    static_assert(NW == 4 || NW == 8, "the workgroup sum below");
    part = as_wave_sum_dpp(part);
    __shared__ float red[NW];
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    float wg_sum = 0.f;      // (tile order and wave order alike for 8 and for 4 waves: the same final sum order)
    if (tid == 0) {
        wg_sum = (red[0] + red[1]) + (red[2] + red[3]);
        if (NW == 8) wg_sum = wg_sum + ((red[4] + red[5]) + (red[6] + red[7]));
    }
    criterion_tail(g, blockIdx.x, wg_sum, tid, red);
}

template <int NW>
__device__ __forceinline__ void criterion_rows(const LinOutK& g, const float* tile, const Tile& t, int tid) {
    constexpr int FPW = 64 / NW;                                // frames per wave
    static_assert(NW == 4 || NW == 8, "the workgroup sum below");
    const int lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int bz = t.bz, m0 = t.m0, rows = 32 * t.tm;
    const int Np = g.N >> 1;                                    // points per contour
    float part = 0.f;
    float tx[FPW], ty[FPW];
    bool in[FPW], valid[FPW];
    const int nl = min(lane, Np - 1);
#pragma unroll
    for (int k = 0; k < FPW; ++k) {
        const int r = wave_u + NW * k;
        const int frame = m0 + r;
        in[k] = r < rows && frame < g.M;
        const int fc = in[k] ? frame : m0;
        const int b = fc / g.T, t_ = fc - b * g.T;
        valid[k] = in[k] && t_ < g.lengths[b];
        const float* tg = g.tgt + (((long)b * g.tgt_T + t_) * g.batch + bz) * g.N;
        tx[k] = tg[nl];
        ty[k] = tg[Np + nl];
    }
#pragma unroll
    for (int k = 0; k < FPW; ++k) {
        if (!in[k]) continue;                       // wave-uniform
        const int r = wave_u + NW * k;
        const long frame = m0 + r;
        float* o = g.out + frame * g.ldo + (long)bz * g.o_batch;
        float* dz = g.dout + frame * g.ldo + (long)bz * g.o_batch;
        if (lane < Np) {
            const float ox = tile[r * ON + lane], oy = tile[r * ON + Np + lane];
            o[lane] = ox;
            o[Np + lane] = oy;
            float gx, gy;
            criterion_point(ox, oy, tx[k], ty[k], valid[k], g.scale, part, gx, gy);
            dz[lane] = gx;
            dz[Np + lane] = gy;
        }
    }
    criterion_sum<NW>(g, part, tid);
}

// The same criterion with row-contiguous 16-byte global accesses (LinOutK::row_epi: N % 4 == 0, out, dout and tgt 16-byte
// aligned; as_set_lin_out_row_epilogue).  Above, a lane owns a point, so a frame costs two dword loads and four dword stores of
// N / 2 live lanes each (200 bytes per instruction at N = 100): 6 x 64 / NW vector-memory instructions per lane and tile.  Here
// the targets come in and out / d(out) leave as float4 chunks of whole rows, two rows per instruction (lanes 0-31 one row, lanes
// 32-63 the next): 3 x 32 / NW instructions, and the arithmetic between them meets its operands in LDS.
// The tile goes in halves of 32 rows (the accumulators' row blocks), so that the 32 KB the kernels own suffice:
//   O[32][ON]  the half's sigmoid outputs, from write_half(IC<h>, O) (the kernel's accumulator layout);
//   T[32][N]   the half's targets, then its d(out), overwritten in place.
// All target loads of both halves are issued before the first store (vector memory operations retire in order).  The
// arithmetic keeps criterion_rows' mapping -- wave w: rows w, w + NW, ...; lane p: point p; rows ascending through the first
// half, then the second -- so every lane adds the same distances in the same order: out, dout and the partial sum are
// criterion_rows' bit for bit.
template <int NW, typename W>
__device__ __forceinline__ void criterion_rows_f4(const LinOutK& g, float* smem, const Tile& t, int tid, W&& write_half) {
    constexpr int FPH = 32 / NW;                                // frames per wave and half (arithmetic)
    constexpr int PPH = 16 / NW;                                // row pairs per wave and half (global accesses)
    const int lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bz = t.bz, m0 = t.m0;
    const int N = g.N, Np = N >> 1;
    const int c4 = 4 * (lane & 31), hw = lane >> 5;             // this lane's chunk of its row; which row of the pair
    const bool chunk = c4 < N;
    float* O = smem;
    float* T = smem + 32 * ON;
    // Lane l works out utterance, time step and validity of tile row l ONCE (one division, one load of lengths[] per wave;
    // criterion_rows does both per frame, and each of its 64 / NW loads of lengths[] is a round trip the next one waits for);
    // a row's values are then read from its lane.  Rows beyond the tile or beyond M take row 0's (valid) target address and are
    // not stored.
    const int rows_in = min(32 * t.tm, g.M - m0);
    const int fc = lane < rows_in ? m0 + lane : m0;
    const int b_l = fc / g.T, t_l = fc - b_l * g.T;
    const int len_l = g.lengths[b_l];
    // rows of pair j of half h: 32 h + 2 * (j * NW + wave) + hw
    bool stored[2][PPH];
    f32x4 tq[2][PPH];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < PPH; ++j) {
            const int r0 = 32 * h + 2 * (j * NW + wave_u);
            stored[h][j] = r0 + hw < rows_in;
            tq[h][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (h >= t.tm) continue;                    // a 32-row tile has no second half
            const long off0 = (((long)__builtin_amdgcn_readlane(b_l, r0) * g.tgt_T + __builtin_amdgcn_readlane(t_l, r0)) * g.batch + bz) * N;
            const long off1 = (((long)__builtin_amdgcn_readlane(b_l, r0 + 1) * g.tgt_T + __builtin_amdgcn_readlane(t_l, r0 + 1)) * g.batch + bz) * N;
            if (chunk) tq[h][j] = *reinterpret_cast<const f32x4*>(g.tgt + (hw ? off1 : off0) + c4);
        }
    const unsigned long long vmask = __ballot(lane < rows_in && t_l < len_l);   // bit r: row r is a frame of its utterance
    float part = 0.f;
    auto half = [&](auto hc) {
        constexpr int h = decltype(hc)::value;
        write_half(hc, O);
#pragma unroll
        for (int j = 0; j < PPH; ++j)
            if (chunk) *reinterpret_cast<f32x4*>(T + (2 * (j * NW + wave_u) + hw) * N + c4) = tq[h][j];
        as_lds_barrier();
#pragma unroll
        for (int k = 0; k < FPH; ++k) {
            const int r = wave_u + NW * k;
            if (32 * h + r >= rows_in) continue;        // wave-uniform
            if (lane < Np) {
                float* tr = T + r * N;
                float gx, gy;
                criterion_point(O[r * ON + lane], O[r * ON + Np + lane], tr[lane], tr[Np + lane], (vmask >> (32 * h + r)) & 1, g.scale, part, gx, gy);
                tr[lane] = gx;
                tr[Np + lane] = gy;
            }
        }
        as_lds_barrier();
#pragma unroll
        for (int j = 0; j < PPH; ++j) {
            const int r = 2 * (j * NW + wave_u) + hw;
            if (chunk && stored[h][j]) {
                const long at = (long)(m0 + 32 * h + r) * g.ldo + (long)bz * g.o_batch + c4;
                *reinterpret_cast<f32x4*>(g.out + at) = *reinterpret_cast<const f32x4*>(O + r * ON + c4);
                *reinterpret_cast<f32x4*>(g.dout + at) = *reinterpret_cast<const f32x4*>(T + r * N + c4);
            }
        }
    };
    half(IC<0>{});
    if (t.tm == 2) {
        as_lds_barrier();                               // the second half reuses O and T
        half(IC<1>{});
    }
    criterion_sum<NW>(g, part, tid);
}

__global__ __launch_bounds__(NT, 4) void lin_out_kernel(LinOutK g) {
    constexpr int TILE = BK * (64 + ON);
    constexpr int RING = NBUF * TILE;            // 9216 floats = 36 KB; the epilogue's [64][ON] tile (32 KB) reuses it
    __shared__ __attribute__((aligned(16))) float smem[RING];
    const Tile t = tile_of<false>(g);
    const int bz = t.bz, m0 = t.m0;
    const float* __restrict__ A = g.A + (long)bz * g.a_batch;
    const float* __restrict__ B = g.B + (long)bz * g.b_batch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave >> 2, wn = wave & 3;
    // DMA sources: A piece = wave & 3 (16 rows x 16 k), B piece = wave (16 output rows x 16 k); chunk swizzle as above
    const int pa = wave & 3;
    const int ra = pa * 16 + (lane >> 2);
    const int a_gc = ((lane & 3) ^ ((ra >> 2) & 3)) * 4;
    const float* a_src = A + (long)min(m0 + ra, g.M - 1) * g.lda + a_gc;
    const int rb = wave * 16 + (lane >> 2);
    const int b_gc = ((lane & 3) ^ ((rb >> 2) & 3)) * 4;
    const float* b_src = B + (long)min(rb, g.b_rows - 1) * g.ldb + b_gc;   // rows beyond the head's own only feed columns >= N
    const unsigned smem_base = as_lds_addr(smem);
    auto issue = [&](int kt) {
        const unsigned base = smem_base + (unsigned)((kt % NBUF) * TILE) * 4u;
        as_glds16(a_src + kt * BK, base + (unsigned)(pa * 1024));
        as_glds16(b_src + kt * BK, base + (unsigned)((BK * 64 + wave * 256) * 4));
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nk = g.K / BK;
    const int swz = (l31 >> 2) & 3;
    const bool active = wm == 0 || t.tm == 2;       // a 32-row tile has one row block: waves 4-7 only help with the DMAs
    issue(0);
    if (nk > 1) issue(1);
    if (nk > 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 2 < nk) issue(kt + 2);
        const float* tile = smem + (kt % NBUF) * TILE;
        const float* a_s = tile + (wm * 32 + l31) * BK;
        const float* b_s = tile + BK * 64 + (wn * 32 + l31) * BK;
        if (active) {
#pragma unroll
            for (int cc = 0; cc < BK / 8; ++cc) {
                const int slot = ((2 * cc + lh) ^ swz) * 4;
                const float4 av = *reinterpret_cast<const float4*>(a_s + slot);
                const float4 bv = *reinterpret_cast<const float4*>(b_s + slot);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
            }
        }
        if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        as_wait_lds();
        __builtin_amdgcn_s_barrier();
    }
    // ---- epilogue.  D[row][col]: col = wn * 32 + l31, row = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh
    const int col = wn * 32 + l31;
    const float bj = (g.bias && col < g.N) ? g.bias[(long)bz * g.bias_batch + col] : 0.f;
    if (g.tgt == nullptr) {
        if (active && col < g.N) store_rows<1>(&acc, g.out + (long)bz * g.o_batch + col, g.ldo, bj, 2, m0 + wm * 32, g.M, 1, lh);
        return;
    }
    // fused criterion: sigmoid outputs through LDS ([64][ON]; every ring read is behind the loop's last barrier)
    if (g.row_epi) {                                // row block h is waves 4 h .. 4 h + 3's
        criterion_rows_f4<8>(g, smem, t, tid, [&](auto hc, float* O) {
            if (wm != decltype(hc)::value) return;
#pragma unroll
            for (int r = 0; r < 16; ++r) O[((r & 3) + 8 * (r >> 2) + 4 * lh) * ON + col] = as_sigmoid(acc[r] + bj);
        });
        return;
    }
    if (active) {
#pragma unroll
        for (int r = 0; r < 16; ++r) smem[(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * ON + col] = as_sigmoid(acc[r] + bj);
    }
    as_lds_barrier();
    criterion_rows<8>(g, smem, t, tid);
}

// The output layer on the bf16 matrix instruction (see lin_s6_kernel): 4 waves, wave w = columns 32 w .. 32 w + 31 of all 64
// rows (two accumulators), A split once per workgroup into the plane image, W3' planes from L2 into registers.  32 KB of
// LDS; built for THREE workgroups per CU (forced to four = 128 VGPRs the 64-row loop reloaded from scratch behind vmcnt(0),
// see lin_s6_plain_kernel).  The bound is a minimum: with both epilogues in the kernel the compiler's own choice is 125 VGPRs
// without scratch (138 with criterion_rows alone), so a fourth workgroup may be resident; the main loop is the same source.
// Epilogue as lin_out_kernel's: criterion_rows / criterion_rows_f4 with 16 instead of 8 frames per wave.
constexpr int LOUT_WPS = 3;    // waves per SIMD = resident workgroups per CU of lin_out_s6_kernel
__global__ __launch_bounds__(256, LOUT_WPS) void lin_out_s6_kernel(LinOutK g) {
    __shared__ __attribute__((aligned(16))) float smem[64 * ON];
    static_assert(64 * ON * 4 >= 2 * S6_BUF, "the epilogue's tile holds both plane images");
    const Tile t = tile_of<true>(g);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    f32x16 acc[2];
    s6_tile<4>(g, t, acc, reinterpret_cast<unsigned char*>(smem), 0, g.K, g.K, tid);
    // ---- epilogue.  D[row][col]: col = wave * 32 + l31, row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh
    const int col = wave * 32 + l31;
    const float bj = (g.bias && col < g.N) ? g.bias[(long)t.bz * g.bias_batch + col] : 0.f;
    if (g.tgt == nullptr) {
        if (col < g.N) store_rows<2>(acc, g.out + (long)t.bz * g.o_batch + col, g.ldo, bj, 2, t.m0, g.M, t.tm, lh);
        return;
    }
    // fused criterion: sigmoid outputs through LDS ([64][ON]; every plane-image read is behind the loop's last barrier)
    if (g.row_epi) {
        criterion_rows_f4<4>(g, smem, t, tid, [&](auto hc, float* O) {
#pragma unroll
            for (int r = 0; r < 16; ++r) O[((r & 3) + 8 * (r >> 2) + 4 * lh) * ON + col] = as_sigmoid(acc[decltype(hc)::value][r] + bj);
        });
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (i < t.tm) smem[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * ON + col] = as_sigmoid(acc[i][r] + bj);
    as_lds_barrier();
    criterion_rows<4>(g, smem, t, tid);
}

// ---- the host half.  lin_plan.cpp decides everything (kernel, planes, tile list, head groups, LDS, k-split, epilogue); here
// the environment is filled, descriptor and plan fields are copied into the kernel argument, and the instantiation the plan
// names is launched.
static_assert(BN == AS_LIN_BN && ON == AS_LIN_ON && BK == AS_LIN_BK && S6_BK == AS_LIN_S6_BK, "lin_plan.cpp plans for these tiles");
static_assert(S6R_MAXK == AS_LIN_SHORT_MAXK && S6_BUF == AS_LIN_S6_IMAGE && 32 * BN * 4 == AS_LIN_STAGE, "lin_plan.cpp sizes the resident image with these");
static_assert(AS_LIN_SLOTS == 2 * 256 && AS_LIN_OUT_SLOTS == 4 * 256 && 2 * AS_LIN_SPREAD == 3 * 256, "slots of the MI355X's 256 CUs");

// as_set_head_short_k (include/artspeech_hip.h)
std::atomic<int> g_short_k{1};
// as_set_lin_out_row_epilogue (include/artspeech_hip.h)
std::atomic<int> g_row_epi{1};

unsigned long long* g_dbg = nullptr;
long g_dbg_max = 0;

// the plan's share of both kernel arguments: the planes where they were taken, and the tile list
template <typename K, typename L>
void plan_args(K& k, const L* a, const as_lin_plan& p) {
    if (p.planes) { k.Bp = a->Bp; k.bp_plane = a->bp_plane; k.bp_batch = a->bp_batch; k.bp_rows = a->bp_rows; }
    k.n_big = p.n_big; k.big_per_batch = p.big_per_batch; k.big_per_batch_rows = p.big_per_batch_rows; k.small_per_batch = p.small_per_batch;
}

// as_lin and its plan as the kernels' argument
LinK lin_args(const as_lin* a, const as_lin_plan& p) {
    LinK k{};
    k.A = a->A; k.lda = a->lda; k.a_batch = a->a_batch;
    k.B = a->B; k.ldb = a->ldb; k.b_batch = a->b_batch;
    k.C = a->C; k.ldc = a->ldc; k.c_batch = a->c_batch;
    k.bias = a->bias; k.bias_batch = a->bias_batch;
    k.M = a->M; k.N = a->N; k.K = a->K; k.ka_valid = a->ka_valid > 0 ? a->ka_valid : a->K; k.batch = a->batch; k.act = a->act;
    k.eps = 1e-5f;
    k.dbg = g_dbg; k.dbg_max = g_dbg_max;
    k.rstd = a->rstd; k.bits = a->bits;
    k.xhat = a->xhat; k.ldx = a->ldx; k.x_batch = a->x_batch; k.rstd_in = a->rstd_in; k.bits_in = a->bits_in;
    plan_args(k, a, p);
    k.groups = p.groups; k.kchunk = p.kchunk;
    return k;
}

}  // namespace

extern "C" void as_lin_debug_stamps(uint64_t* buf, int64_t max_workgroups) {
    g_dbg = (unsigned long long*)buf;
    g_dbg_max = buf ? max_workgroups : 0;
}

extern "C" void as_set_head_short_k(int32_t on) { g_short_k.store(on ? 1 : 0, std::memory_order_relaxed); }

extern "C" void as_set_lin_out_row_epilogue(int32_t on) { g_row_epi.store(on ? 1 : 0, std::memory_order_relaxed); }

// see gemm_internal.h
as_lin_env as_lin_env_of(hipStream_t st, bool ask_counter) {
    as_lin_env e{};
    e.arith = as_matrix_arith();
    e.short_k = g_short_k.load(std::memory_order_relaxed) != 0;
    e.row_epi = g_row_epi.load(std::memory_order_relaxed) != 0;
    e.counter = ask_counter && as_arrival_counter(st) != nullptr;
    e.lds_limit = AS_LIN_LDS_MI355X;
    return e;
}

// see gemm_internal.h.  Returns 1 if launched, 0 if the arguments are outside what the kernels are built for (the caller
// then takes the general GEMM + row kernels), < 0 on a launch error.
int as_lin_try(const as_lin* a, hipStream_t st) {
    const as_lin_env env = as_lin_env_of(st);
    as_lin_plan p;
    as_lin_plan_make(a, &env, &p);
    if (p.family == AS_LIN_NONE) return 0;
    const LinK k = lin_args(a, p);
    const dim3 grid((unsigned)p.tiles);
    int rc = 0;
    switch (p.family) {
        case AS_LIN_LNF_SHARED:
            // (more than the 64 KB a kernel has without asking; the planner has kept it within the device's limit)
            if (p.lds > 64 * 1024 && as_allow_dynamic_lds(lin_s6_lnf_shared_kernel, p.lds) != hipSuccess) {
                as_set_error("as_lin_s6_lnf_shared: %d bytes of dynamic LDS refused", p.lds);
                return -1;
            }
            hipLaunchKernelGGL(lin_s6_lnf_shared_kernel, grid, dim3(NT), p.lds, st, k);
            break;
        case AS_LIN_LNB_SHORT: hipLaunchKernelGGL(lin_s6_lnb_short_kernel, grid, dim3(NT), 0, st, k); break;
        case AS_LIN_S6:   // B as planes: the products run on the bf16 matrix instruction
            as_exactly<EPI_LNF, EPI_LNB, EPI_PLAIN>(p.epi, &rc, [&](auto e) {
                hipLaunchKernelGGL((lin_s6_kernel<decltype(e)::value>), grid, dim3(NT), 0, st, k);
                return 0;
            });
            break;
        default:          // AS_LIN_F32; 2 epi + b_kc: the LayerNorm epilogues exist for one orientation of B each
            as_exactly<2 * EPI_LNF + 1, 2 * EPI_LNB, 2 * EPI_PLAIN + 1, 2 * EPI_PLAIN>(2 * p.epi + p.b_kc, &rc, [&](auto c) {
                constexpr int C = decltype(c)::value;
                hipLaunchKernelGGL((lin_f32_kernel<64, C % 2 == 1, C / 2>), grid, dim3(NT), 0, st, k);
                return 0;
            });
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        as_set_error("as_lin_try: launch failed: %s", hipGetErrorString(e));
        return -1;
    }
    return 1;
}

// see gemm_internal.h
int as_lin_plain_s6(const as_lin* a, int ksplit, long c_split, hipStream_t st, int waves_per_simd) {
    const as_lin_env env = as_lin_env_of(st);
    as_lin_plan p;
    as_lin_plain_plan_make(a, ksplit, waves_per_simd, &env, &p);
    if (p.family == AS_LIN_NONE) return 0;
    LinK k = lin_args(a, p);
    k.c_split = c_split;
    const dim3 grid((unsigned)p.tiles, p.ksplit);
    if (p.nw == 4 && p.wps == 2) hipLaunchKernelGGL((lin_s6_plain_kernel<4, 2>), grid, dim3(256), 0, st, k);
    else if (p.nw == 4) hipLaunchKernelGGL((lin_s6_plain_kernel<4, 4>), grid, dim3(256), 0, st, k);
    else hipLaunchKernelGGL((lin_s6_plain_kernel<8, 4>), grid, dim3(512), 0, st, k);
    AS_LAUNCH_CHECK("as_lin_plain_s6");
    return 1;
}

// Output layer of the heads, optionally with the masked Euclidean criterion and its gradient fused in (see lin_out_kernel).
// 1 = launched (fused: *n_partials workgroup sums were written to `partial`), 0 = not a case, < 0 = error.
int as_lin_out_try(const as_lin_out* a, int* n_partials, hipStream_t st) {
    // (asking for the stream's arrival counter creates it: only a launch that can use one asks)
    const as_lin_env env = as_lin_env_of(st, a->tgt && a->loss);
    as_lin_plan p;
    as_lin_out_plan_make(a, &env, &p);
    if (p.family == AS_LIN_NONE) return 0;
    LinOutK k{};
    k.A = a->A; k.lda = a->lda; k.a_batch = a->a_batch;
    k.B = a->B; k.ldb = a->ldb; k.b_batch = a->b_batch; k.b_rows = a->b_rows;
    k.bias = a->bias; k.bias_batch = a->bias_batch;
    k.out = a->out; k.ldo = a->ldo; k.o_batch = a->o_batch;
    k.M = a->M; k.N = a->N; k.K = a->K; k.batch = a->batch;
    k.tgt = a->tgt; k.tgt_T = a->tgt_T; k.lengths = a->lengths; k.T = a->T; k.scale = a->scale; k.dout = a->dout; k.partial = a->partial;
    plan_args(k, a, p);
    k.row_epi = p.row_epi;
    if (p.sums_loss) { k.counter = as_arrival_counter(st); k.loss = a->loss; }
    if (n_partials) *n_partials = p.partials;
    if (p.family == AS_LIN_OUT_S6) hipLaunchKernelGGL(lin_out_s6_kernel, dim3((unsigned)p.tiles), dim3(256), 0, st, k);
    else hipLaunchKernelGGL(lin_out_kernel, dim3((unsigned)p.tiles), dim3(NT), 0, st, k);
    AS_LAUNCH_CHECK(p.planes ? "as_lin_out_s6" : "as_lin_out");
    return 1;
}

// ---- include/artspeech_hip.h: as_linear_fwd
extern "C" int64_t as_linear_planes_floats(int32_t N, int32_t K) {
    int bn, nb;
    if (N < 1 || K < 1 || !as_linear_blocks(N, &bn, &nb)) return 0;
    return as_round_up(as_planes_floats(nb, bn, (int)as_round_up(K, 32)), 64);
}

extern "C" int as_linear_fwd(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* out, int64_t ldo,
                             int32_t M, int32_t N, int32_t K, int32_t act, float* planes_ws, void* stream) {
    AS_REQUIRE(A && W && out && M > 0 && N > 0 && K > 0 && lda >= K && ldw >= K && ldo >= N && act >= 0 && act <= 2, AS_ERR_BAD_ARG,
               "as_linear_fwd: bad argument");
    hipStream_t st = (hipStream_t)stream;
    int bn, nb;
    if (as_matrix_arith() == AS_ARITH_BF16X6 && planes_ws && K % S6_BK == 0 && lda % 4 == 0 && as_linear_blocks(N, &bn, &nb) &&
        as_aligned16(planes_ws)) {
        const int rows_last = N - (nb - 1) * bn;   // (nb > 1: whole blocks)
        as_planes_job j{W, ldw, 1, (long)bn * ldw, nb, nb > 1 ? bn : rows_last, K, bn, K, reinterpret_cast<uint16_t*>(planes_ws)};
        AS_TRY(as_emit_planes(&j, 1, st));
        as_lin l{};
        l.A = A; l.lda = lda;
        l.Bp = reinterpret_cast<const uint16_t*>(planes_ws); l.bp_rows = bn; l.bp_batch = as_planes_batch_stride(bn, K); l.bp_plane = nb * l.bp_batch;
        l.C = out; l.ldc = ldo; l.c_batch = bn;
        l.bias = bias; l.bias_batch = bn; l.act = act;
        l.M = M; l.N = nb > 1 ? bn : N; l.K = K; l.batch = nb;
        const int took = as_lin_plain_s6(&l, 1, 0, st);
        AS_REQUIRE(took >= 0, took, "as_linear_fwd: launch failed");
        if (took) return 0;
    }
    as_gemm g{};
    g.A = A; g.B = W; g.C = out; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.a_i = lda; g.a_k = 1; g.b_j = ldw; g.b_k = 1; g.ldc = ldo; g.batch = 1; g.act = act;
    // no scratch for planes: both operands split inside the kernel where gemm_s6.hip takes the shape; a plane kernel that declined
    // stays on the exact general kernel
    g.precision = planes_ws ? 0 : 3;
    return as_gemm_f32(&g, st);
}
