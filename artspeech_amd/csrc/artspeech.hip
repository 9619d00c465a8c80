// Composite entry points: the flat parameter layout, the workspace carve and the launch sequences of
// ArtSpeech / SimpleArtSpeech forward + backward and of the stacked ArticulatorPredictor heads.
// This is the native "runtime" of the path: Python hands over pointers once per step; every kernel of
// the step is enqueued from here on one HIP stream (graph-capturable: no allocation, no sync).
//
// Design notes (reference lines: encoder_decoder/models.py):
//  * embedding (:135) + layer-0 input projection are folded into a [V][2][3H] row table (one tiny
//    GEMM per step); the GRU kernel gathers table rows by token id, so neither the embedded sequence
//    nor its projection is ever materialised.  Backward: per-token segment sum -> two tiny GEMMs.
//  * every LayerNorm of the heads (:11,14,17) is applied affine-free (x_hat) and its gamma/beta are
//    folded into the following Linear (W' = W.diag(gamma), b' = b + W.beta).  The first LayerNorm's
//    x_hat is then shared by all A heads (same input row), and head GEMM 1 becomes ONE GEMM with
//    N = A*256 columns.  The backward unfolds dW', db' into dW, dgamma, dbeta, db exactly.
//  * heads are batched over A with strided-batched GEMMs on [rows][A][256] activations; the last GEMM
//    writes sigmoid(.) straight into the (B, T, A, 2, N) output (:141-145).
//
// Where to look in the head stack:
//  * head_ws carves the workspace, head_plane_jobs states the geometry of every bfloat16 plane image, and head_stack
//    turns both into one HeadLayer per Linear: where its input, folded weight, planes, gradients and parameters live.
//    head_fold, the forward, the input-gradient chain and the weight gradients all read a layer's operands from there.
//  * lin_fwd / lin_bwd pose a layer as an as_lin; lin_or_general launches the fused kernel for it or, when that declines,
//    the general GEMM + row kernel that lin_general derives from the same as_lin.
//  * wgrad / wgrad1 (and the model's backward for the trunk) pose each weight-gradient problem once: as_wgrad_multi takes
//    them as jobs, and the single-problem route hands the same as_gemm to as_gemm_f32 with slab and CU budget filled in.
//  * gemm_nt / gemm_nn / gemm_tn only set an orientation's strides; everything else is set by field name at the call site.
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "as_launch.h"
#include "gemm_internal.h"
#include "rowops.h"

namespace {

constexpr int D = AS_HEAD_HIDDEN;
constexpr int64_t SLAB_FLOATS = 16LL << 20;  // 64 MB of split-K partial tiles per stream
constexpr int64_t SLAB2_FLOATS = 28LL << 20; // first side stream: the partial tiles of ALL head weight gradients in one launch

struct Carve {
    int64_t off = 0;
    int64_t take(int64_t n) {
        const int64_t o = off;
        off += as_round_up(n, 64);
        return o;
    }
};

constexpr int OUT_BN = 128;   // column tile of the output layer's kernel (lin_out): rows of the W3' planes per head
enum { W1P, W2P, W3P, W2TP, W3TP, W1TP, N_PLANES };   // the plane images of the folded weights, in carve and emission order

// in / out features per head of head layer i (0..2), and the rows per head of its folded weight (rows N .. Npad-1 are zeros)
struct LayerDims { int K, N, Npad; };
LayerDims layer_dims(const as_dims& d, int i) {
    const int O = 2 * d.n_samp;
    if (i < 2) return {i == 0 ? d.hidden : D, D, D};
    return {D, O, (int)as_round_up(O, 32)};
}

struct HeadWs {  // offsets in floats relative to the head workspace base; [i]: head layer i
    int64_t x[3], rstd[3], bits[3], wf[3], bf[3], dz[3], dwf[3], planes[N_PLANES];   // see HeadLayer
    int64_t dxhat, slab, slab2, slab3, lpart, lpart_n, total;
};

// The folded weights as bfloat16 planes (as_emit_planes) for the split-arithmetic kernels: the source view and the padded
// geometry of each image, stated here and nowhere else (B and out are filled in by head_stack).  Forward orientation
// [rows = out features][k = in features] and, for the input-gradient chain (d(x_hat) = dz . W': the reduction runs over W'
// rows), transposed [rows = in features][k = out features].
void head_plane_jobs(const as_dims& d, as_planes_job j[N_PLANES]) {
    const int A = d.n_art, H = d.hidden, O = 2 * d.n_samp, Opad = (int)as_round_up(O, 32);
    //         B, n_stride, k_stride, batch_stride, batch, N, K, rows_pad, Kpad, out
    j[W1P] = {nullptr, H, 1, (long)D * H, A, D, H, D, (int)as_round_up(H, 32), nullptr};
    j[W2P] = {nullptr, D, 1, (long)D * D, A, D, D, D, D, nullptr};
    j[W3P] = {nullptr, D, 1, (long)Opad * D, A, O, D, (int)as_round_up(O, OUT_BN), D, nullptr};
    j[W2TP] = {nullptr, 1, D, (long)D * D, A, D, D, D, D, nullptr};
    j[W3TP] = {nullptr, 1, D, (long)Opad * D, A, D, O, D, Opad, nullptr};
    // d(x_hat) = dz1 . W1' summed over the heads: ONE image, rows = the H inputs, k = (head, feature)
    j[W1TP] = {nullptr, 1, H, 0, 1, H, A * D, (int)as_round_up(H, 128), A * D, nullptr};
}

HeadWs head_ws(const as_dims& d, int64_t rows) {
    const int64_t A = d.n_art;
    const LayerDims n[3] = {layer_dims(d, 0), layer_dims(d, 1), layer_dims(d, 2)};
    Carve c;
    HeadWs w{};
    w.x[0] = c.take(rows * n[0].K);
    w.rstd[0] = c.take(rows);
    for (int i = 0; i < 3; ++i) {
        w.wf[i] = c.take(A * n[i].Npad * n[i].K);
        w.bf[i] = c.take(A * n[i].N);
    }
    for (int i = 1; i < 3; ++i) {
        w.x[i] = c.take(rows * A * n[i].K);
        w.rstd[i] = c.take(rows * A);
    }
    for (int i = 2; i >= 0; --i) w.dz[i] = c.take(rows * A * n[i].N);
    w.dxhat = c.take(rows * n[0].K);
    for (int i = 0; i < 3; ++i) w.dwf[i] = c.take(A * n[i].N * n[i].K);
    w.slab = c.take(SLAB_FLOATS);   // split-K partial tiles of the weight-gradient GEMMs (main stream)
    w.slab2 = c.take(SLAB2_FLOATS); // same, for GEMMs issued on the side stream
    w.slab3 = c.take(SLAB_FLOATS);  // same, second side stream
    for (int i = 1; i < 3; ++i) w.bits[i] = c.take(rows * A * (n[i].K / 64) * 2);   // 64-bit words, 16-byte aligned
    // workgroup partial sums of the fused criterion (one per output-layer tile), or of the separate criterion kernel
    w.lpart_n = std::max<int64_t>((rows / 32 + 2) * A, as_euclid_masked_partials());
    w.lpart = c.take(w.lpart_n);
    as_planes_job pj[N_PLANES];
    head_plane_jobs(d, pj);
    for (int i = 0; i < N_PLANES; ++i) w.planes[i] = c.take(as_planes_floats(pj[i].batch, pj[i].rows_pad, pj[i].Kpad));
    w.total = c.off;
    return w;
}

// One Linear of the heads with the LayerNorm in front of it folded in: where its operands live.  What layer i produces
// (x_hat, 1 / std, ReLU bits) is the input of layer i + 1; the output layer writes the caller's `out`.
struct HeadLayer : LayerDims {
    float* x; long ldx, x_batch;   // normalised input [rows][A][K] (layer 1: [rows][K] shared by all heads, batch stride 0),
    float* rstd;                   // its 1 / std per row and head,
    unsigned long long* bits;      // and the ReLU mask of what was normalised: one bit per element (layer 1: none)
    float* wf; float* bf;          // folded weight [A][Npad][K] and bias [A][N]
    as_planes_job fwd, tr;         // wf as bfloat16 planes, forward and transposed (head_plane_jobs)
    // d loss / d(pre-activation) [rows][A][N].  Layers 1, 2: the forward's general route (lin_general) leaves the
    // pre-normalisation activations here -- nothing touches it before the backward; the fused route never stores them.
    float* dz; long ldz;
    float* dwf;                    // gradient of wf [A][N][K]
    int64_t w, b, ln_g, ln_b;      // the unfolded layer in the flat parameter / gradient buffers (as_layout)
    long w_batch() const { return (long)Npad * K; }
};
struct HeadStack {
    int A, H, O, R, n_samp;        // heads, input width, outputs per head (2 n_samp), rows
    float* ws; HeadWs w;           // the carve: dxhat, the slabs and the criterion's partials belong to no layer
    HeadLayer l[3];
};

HeadStack head_stack(const as_dims& d, const as_layout& L, int64_t rows, float* ws) {
    HeadStack s{};
    s.A = d.n_art; s.H = d.hidden; s.n_samp = d.n_samp; s.O = 2 * d.n_samp; s.R = (int)rows; s.ws = ws; s.w = head_ws(d, rows);
    const HeadWs& w = s.w;
    as_planes_job pj[N_PLANES];
    head_plane_jobs(d, pj);
    for (int i = 0; i < N_PLANES; ++i) pj[i].out = reinterpret_cast<uint16_t*>(ws + w.planes[i]);
    const int tr[3] = {W1TP, W2TP, W3TP};   // (forward images: W1P + i)
    const int64_t pw[3] = {L.w1, L.w2, L.w3}, pb[3] = {L.b1, L.b2, L.b3}, pg[3] = {L.ln1_g, L.ln2_g, L.ln3_g}, pbt[3] = {L.ln1_b, L.ln2_b, L.ln3_b};
    for (int i = 0; i < 3; ++i) {
        HeadLayer& l = s.l[i];
        static_cast<LayerDims&>(l) = layer_dims(d, i);
        l.x = ws + w.x[i]; l.ldx = i ? (long)s.A * l.K : l.K; l.x_batch = i ? l.K : 0;
        l.rstd = ws + w.rstd[i]; l.bits = i ? reinterpret_cast<unsigned long long*>(ws + w.bits[i]) : nullptr;
        l.wf = ws + w.wf[i]; l.bf = ws + w.bf[i];
        l.fwd = pj[W1P + i]; l.tr = pj[tr[i]]; l.fwd.B = l.tr.B = l.wf;
        l.dz = ws + w.dz[i]; l.ldz = (long)s.A * l.N; l.dwf = ws + w.dwf[i];
        l.w = pw[i]; l.b = pb[i]; l.ln_g = pg[i]; l.ln_b = pbt[i];
    }
    return s;
}

struct ModelWs {
    int64_t tokflag, tab0, y0, y0d, g0, xp1, y1, g1, lin, head, dy1, dgi1, dgh1, dy0, dgi0, dgh0, dtab0, total;
};

ModelWs model_ws(const as_dims& d, int64_t B, int64_t T) {
    const int64_t R = B * T, H = d.hidden, V = d.vocab;
    Carve c;
    ModelWs w{};
    w.tokflag = c.take(64);   // first word (int32): ids outside [0, V) seen by the last as_artspeech_fwd on this workspace
    if (!d.simple) {
        w.tab0 = c.take(V * 6 * H);
        w.y0 = c.take(R * 2 * H);
        w.y0d = c.take(R * 2 * H);  // layer-0 output after inter-layer dropout (training with p > 0)
        w.g0 = c.take(R * 8 * H);
        w.xp1 = c.take(R * 6 * H);
        w.y1 = c.take(R * 2 * H);
        w.g1 = c.take(R * 8 * H);
        w.dy1 = c.take(R * 2 * H);
        w.dgi1 = c.take(R * 6 * H);
        w.dgh1 = c.take(R * 6 * H);
        w.dy0 = c.take(R * 2 * H);
        w.dgi0 = c.take(R * 6 * H);
        w.dgh0 = c.take(R * 6 * H);
        w.dtab0 = c.take(V * 6 * H);
    } else {
        w.tab0 = c.take(V * H);   // relu(Emb Wl^T + bl) per token
        w.dtab0 = c.take(V * H);
        w.y0 = c.take(R * d.embed);   // training with dropout p > 0: the embedded frames after dropout ...
        w.dy0 = c.take(R * d.embed);  // ... and the gradient that reaches them
    }
    w.lin = c.take(R * H);
    w.head = c.take(head_ws(d, R).total);
    w.total = c.off;
    return w;
}

int check_dims(const as_dims* d, const char* who) {
    AS_REQUIRE(d, AS_ERR_BAD_ARG, "%s: null dims", who);
    AS_REQUIRE(d->vocab > 0 && d->n_art > 0 && d->embed > 0 && d->hidden > 0 && d->n_samp > 0, AS_ERR_BAD_ARG,
               "%s: non-positive dimension (V=%d A=%d E=%d H=%d N=%d)", who, d->vocab, d->n_art, d->embed, d->hidden, d->n_samp);
    AS_REQUIRE(d->hidden <= 512, AS_ERR_UNSUPPORTED, "%s: hidden size %d > 512", who, d->hidden);
    // hidden sizes 32 / 64 / 128 run the register-resident recurrence kernels, any other multiple of 4 (16-byte rows) the plain
    // ones of gru.hip (several times slower per step)
    if (!d->simple)
        AS_REQUIRE(d->hidden % 4 == 0, AS_ERR_UNSUPPORTED, "%s: GRU hidden size %d is not a multiple of 4", who, d->hidden);
    return 0;
}

// as_gemm builders: one problem (batch 1) with the orientation's strides set (x_kc: the operand is reduction-contiguous).
// Everything else -- bias, act, batch and its strides, the time shift of B, colsum, the split-K slab, cu_budget -- is set by
// field name where the GEMM is posed.
as_gemm gemm_of(const float* A, long lda, bool a_kc, const float* B, long ldb, bool b_kc, float* C, long ldc, int M, int N, int K) {
    as_gemm g{};
    g.A = A; g.B = B; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.batch = 1;
    g.a_i = a_kc ? lda : 1; g.a_k = a_kc ? 1 : lda; g.b_j = b_kc ? ldb : 1; g.b_k = b_kc ? 1 : ldb;
    return g;
}
// C = act(A . B^T + bias): both operands reduction-contiguous
as_gemm gemm_nt(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K) {
    return gemm_of(A, lda, true, B, ldb, true, C, ldc, M, N, K);
}
// C[M][N] = A[M][K] . B[K][N]   (input gradient: reduction over the rows of B)
as_gemm gemm_nn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K) {
    return gemm_of(A, lda, true, B, ldb, false, C, ldc, M, N, K);
}
// C[M][N] = A[K][M]^T . B[K][N]   (weight gradient: reduction over the rows of both; g.colsum: the column sums of A, i.e. the
// bias gradient that goes with it, [batch][M])
as_gemm gemm_tn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K) {
    return gemm_of(A, lda, false, B, ldb, false, C, ldc, M, N, K);
}
// One stream of a call with what a launch on it needs: the stream's own split-K slab and its size, and the CUs the heads'
// weight gradients are planned with there (0 = all; 192 beside a recurrence, whose 2 * B workgroups hold 64 CUs)
struct Lane { hipStream_t stream; float* slab; long slab_floats; int cu_budget; };
// few output tiles under a long reduction: split K over the lane's slab (every slab of the carve holds SLAB_FLOATS or more; the
// split factor depends on the size stated).  cu_budget: CUs the launch can count on (0 = all)
int run_split_k(as_gemm g, const Lane& ln, int cu_budget = 0) {
    g.splitk_ws = ln.slab; g.splitk_ws_floats = SLAB_FLOATS; g.cu_budget = cu_budget;
    return as_gemm_f32(&g, ln.stream);
}

// hand a plane image to the kernel that reads it (as_lin.Bp / as_lin_out.Bp)
template <typename Lin>
void use_planes(Lin& a, const as_planes_job& p) {
    a.Bp = p.out; a.bp_rows = p.rows_pad; a.bp_batch = as_planes_batch_stride(p.rows_pad, p.Kpad); a.bp_plane = p.batch * a.bp_batch;
}

// fold the LayerNorm affines into the head weights (depends on the parameters only: can run early / elsewhere)
int head_fold(const HeadStack& s, const float* P, hipStream_t st) {
    for (const HeadLayer& l : s.l)
        AS_STEP("head.fold", st, as_fold(P + l.w, P + l.ln_g, P + l.ln_b, P + l.b, l.wf, l.bf, s.A, l.N, l.K, st, l.Npad));
    // the folded weights as bfloat16 planes.  Emitted for every hidden size and in both arithmetics: the head layers hand them
    // to the split kernels whatever H is, and the arithmetic is read at each launch, so a backward may run in the split
    // arithmetic after a forward in the exact one.
    const as_planes_job j[N_PLANES] = {s.l[0].fwd, s.l[1].fwd, s.l[2].fwd, s.l[1].tr, s.l[2].tr, s.l[0].tr};
    AS_STEP("head.planes", st, as_emit_planes(j, N_PLANES, st));
    return 0;
}

// Layer i forward as the fused kernels see it.  i < 2: Linear + ReLU + the next LayerNorm in one kernel per (64 frames,
// head), which writes layer i + 1's input (lin_f32.hip); i == 2: Linear (x_coords | y_coords) + sigmoid into out[rows][A][2][N].
as_lin lin_fwd(const HeadStack& s, int i, float* out = nullptr) {
    const HeadLayer& l = s.l[i];
    as_lin a{};
    a.A = l.x; a.lda = l.ldx; a.a_batch = l.x_batch;
    a.B = l.wf; a.ldb = l.K; a.b_batch = l.w_batch(); a.b_kc = 1;
    a.bias = l.bf; a.bias_batch = l.N;
    a.M = s.R; a.N = l.N; a.K = l.K; a.batch = s.A;
    if (i == 2) {
        a.C = out; a.ldc = (long)s.A * l.N; a.c_batch = l.N; a.act = 2; a.epi = 0;
        return a;
    }
    const HeadLayer& y = s.l[i + 1];
    a.C = y.x; a.ldc = y.ldx; a.c_batch = y.x_batch; a.epi = 1; a.rstd = y.rstd; a.bits = y.bits;
    if (l.K % 32 == 0) use_planes(a, l.fwd);
    return a;
}
// Input gradient of layer i (2, 1): d(x_hat) = dz . W' through the LayerNorm and the ReLU behind layer i - 1 in one kernel,
// which writes layer i - 1's dz.  The reduction runs over Npad (the folded weights' rows N .. Npad-1 are zeros; dz is read
// up to N); the ReLU masks come as bit words (32 B per row).
as_lin lin_bwd(const HeadStack& s, int i, const float* dz) {
    const HeadLayer &l = s.l[i], &to = s.l[i - 1];
    as_lin a{};
    a.A = dz; a.lda = l.ldz; a.a_batch = l.N;
    a.B = l.wf; a.ldb = l.K; a.b_batch = l.w_batch(); a.b_kc = 0;
    a.C = to.dz; a.ldc = to.ldz; a.c_batch = to.N;
    a.M = s.R; a.N = l.K; a.K = l.Npad; a.ka_valid = l.N; a.batch = s.A; a.epi = 2;
    a.xhat = l.x; a.ldx = l.ldx; a.x_batch = l.x_batch; a.rstd_in = l.rstd; a.bits_in = l.bits;
    use_planes(a, l.tr);
    return a;
}

// What runs when the fused kernel declines, derived from the SAME as_lin: the general GEMM, then the epilogue's row kernel
// (which takes C as [M * batch][N], the heads' layout).  epi 0: C = act(A . B^T + bias).  epi 1: pre = relu(A . B^T + bias),
// then as_normalize_fwd: pre -> C, rstd, bits.  epi 2: C = A . B over the ka_valid rows of B, then as_normalize_bwd in place.
// A batch that is one problem is posed as one: when every member reads the same A (a_batch == 0) and B, C and the bias are
// contiguous across the batch (b_batch == N * ldb, c_batch == N, bias_batch == N), it is ONE GEMM over batch * N columns
// (layer 1: A * 256), not `batch` GEMMs of N.
int lin_general(const as_lin& a, float* pre, const char* gemm_phase, const char* norm_phase, hipStream_t st) {
    as_gemm g = a.b_kc ? gemm_nt(a.A, a.lda, a.B, a.ldb, a.epi == 1 ? pre : a.C, a.ldc, a.M, a.N, a.K)
                       : gemm_nn(a.A, a.lda, a.B, a.ldb, a.C, a.ldc, a.M, a.N, a.ka_valid > 0 ? a.ka_valid : a.K);
    g.bias = a.bias;
    g.act = a.epi == 1 ? 1 : a.act;
    if (a.b_kc && a.a_batch == 0 && a.b_batch == a.N * a.ldb && a.c_batch == a.N && a.bias_batch == a.N) {
        g.N = a.batch * a.N;
    } else {
        g.batch = a.batch; g.a_batch = a.a_batch; g.b_batch = a.b_batch; g.c_batch = a.c_batch; g.bias_batch = a.bias_batch;
    }
    AS_STEP(gemm_phase, st, as_gemm_f32(&g, st));
    const long rows = (long)a.M * a.batch;
    if (a.epi == 1) AS_STEP(norm_phase, st, as_normalize_fwd(pre, a.C, a.rstd, rows, a.N, st, a.bits));
    if (a.epi == 2) AS_STEP(norm_phase, st, as_normalize_bwd(a.C, a.xhat, a.rstd_in, nullptr, a.C, rows, a.N, st, a.bits_in));
    return 0;
}
// One head layer: the fused kernel, else lin_general.  pre (epi 1): scratch for the general route's pre-normalisation values.
int lin_or_general(const as_lin& a, float* pre, const char* gemm_phase, const char* norm_phase, const char* what, hipStream_t st) {
    int took;
    {
        AS_PROF(gemm_phase, st);
        took = as_lin_try(&a, st);
        AS_REQUIRE(took >= 0, took, "%s: launch failed", what);
    }
    return took ? 0 : lin_general(a, pre, gemm_phase, norm_phase, st);
}

// crit (optional): the training criterion fused into the output layer (as_opts.loss_*; lengths / T of the batch)
struct Criterion { const float* tgt; long tgt_T; const int* lengths; int T; float scale; float* loss; float* dout; };

int head_fwd_impl(const HeadStack& s, const float* x, float* out, hipStream_t st, const Criterion* crit = nullptr) {
    AS_STEP("head.norm0", st, as_normalize_fwd(x, s.l[0].x, s.l[0].rstd, s.R, s.H, st));
    // Linear 1 (all heads read the shared x_hat) and Linear 2, each with its ReLU and the LayerNorm behind it
    AS_TRY(lin_or_general(lin_fwd(s, 0), s.l[0].dz, "head.gemm1", "head.norm1", "head gemm1", st));
    AS_TRY(lin_or_general(lin_fwd(s, 1), s.l[1].dz, "head.gemm2", "head.norm2", "head gemm2", st));
    // The output layer's chain: lin_out (64 x 128-column tiles of one head each, four workgroups per CU; with `crit` the masked
    // Euclidean criterion and its gradient ride in the epilogue), else the 256-column kernel, else the general GEMM
    const as_lin l3 = lin_fwd(s, 2, out);
    float* lpart = s.ws + s.w.lpart;
    int took;
    bool crit_done = false;
    {
        AS_PROF("head.gemm3", st);
        as_lin_out lo{};
        lo.A = l3.A; lo.lda = l3.lda; lo.a_batch = l3.a_batch;
        lo.B = l3.B; lo.ldb = l3.ldb; lo.b_batch = l3.b_batch; lo.b_rows = s.l[2].Npad;
        lo.bias = l3.bias; lo.bias_batch = l3.bias_batch;
        lo.out = l3.C; lo.ldo = l3.ldc; lo.o_batch = l3.c_batch;
        lo.M = l3.M; lo.N = l3.N; lo.K = l3.K; lo.batch = l3.batch;
        use_planes(lo, s.l[2].fwd);
        int n_part = 0;
        if (crit) {
            lo.tgt = crit->tgt; lo.tgt_T = crit->tgt_T; lo.lengths = crit->lengths; lo.T = crit->T; lo.scale = crit->scale;
            lo.dout = crit->dout; lo.partial = lpart; lo.partial_capacity = s.w.lpart_n; lo.loss = crit->loss;
        }
        took = as_lin_out_try(&lo, &n_part, st);
        AS_REQUIRE(took >= 0, took, "head gemm3: launch failed");
        if (took && crit && n_part > 0) AS_TRY(as_loss_final(lpart, n_part, crit->scale, crit->loss, st));   // (0: summed in the kernel)
        crit_done = took && crit;
        if (!took) {
            took = as_lin_try(&l3, st);
            AS_REQUIRE(took >= 0, took, "head gemm3: launch failed");
        }
    }
    if (!took) AS_TRY(lin_general(l3, nullptr, "head.gemm3", nullptr, st));
    if (crit && !crit_done) {
        // the output-layer kernel declined (more than 128 outputs per head, fewer than 4, odd strides): the criterion as its own
        // kernel on the stored contours -- same loss, same d loss / d(pre-sigmoid), one pass more
        AS_STEP("loss", st, as_euclid_masked_fwd_bwd_presigmoid(out, crit->tgt, crit->tgt_T, crit->lengths, (int32_t)(s.R / crit->T), crit->T, s.A,
                                                               s.n_samp, crit->scale, crit->loss, crit->dout, lpart, st));
    }
    return 0;
}

// Backward of the heads in two parts so that the caller can put them on different streams:
//  head_bwd_dx : the input-gradient chain (critical path towards the GRU backward)
//  head_bwd_dw : weight/bias gradients + LayerNorm-affine unfold (only consumes what the chain left in ws)
// relu_src: optional [rows][H] activation whose ReLU produced x (its mask is fused into the last step)
// presig: dout already is the gradient w.r.t. the pre-sigmoid activations (as_opts.dout_presigmoid): read in place
int head_bwd_dx(const HeadStack& s, const float* out, const float* dout, float* dx, const float* relu_src, hipStream_t st,
                bool presig = false) {
    const int H = s.H, R = s.R;
    const HeadLayer& l1 = s.l[0];
    float* slab = s.ws + s.w.slab;
    float* dxhat = s.ws + s.w.dxhat;
    if (!presig) AS_STEP("headb.sigmoid", st, as_sigmoid_bwd(out, dout, s.l[2].dz, (long)R * s.l[2].ldz, st));
    AS_TRY(lin_or_general(lin_bwd(s, 2, presig ? dout : s.l[2].dz), nullptr, "headb.dx3", "headb.norm2", "head dx3", st));
    AS_TRY(lin_or_general(lin_bwd(s, 1, s.l[1].dz), nullptr, "headb.dx2", "headb.norm1", "head dx2", st));
    // d(x_hat) = dz1 . W1' summed over the heads: N = H columns under an A * 256-long reduction.  Split arithmetic: 64 x 128
    // tiles, the reduction cut into chunks whose partial sums the LayerNorm backward below adds (as_lin_plain_s6); else the
    // general kernel (100 x 2 tiles of 64 x 64, split K over the main-stream slab).  The planner (lin_plan.h) says ahead of the
    // launch whether the kernel takes it and how many slabs it will write: they must fit the slab.
    int dx1_slabs = 0;
    as_lin l{};
    l.A = l1.dz; l.lda = l1.ldz;
    use_planes(l, l1.tr);
    l.C = slab; l.ldc = H;
    l.M = R; l.N = H; l.K = (int)l1.ldz; l.batch = 1;
    const as_lin_env env = as_lin_env_of(st);
    as_lin_plan plan;
    as_lin_plain_plan_make(&l, AS_LIN_KSPLIT_AUTO, 2, &env, &plan);
    if (plan.family != AS_LIN_NONE && (int64_t)plan.ksplit * R * H <= SLAB_FLOATS) {
        AS_PROF("headb.dx1", st);
        const int took1 = as_lin_plain_s6(&l, AS_LIN_KSPLIT_AUTO, (long)R * H, st, 2);
        AS_REQUIRE(took1 >= 0, took1, "head dx1: launch failed");
        if (took1) dx1_slabs = plan.ksplit;
    }
    if (!dx1_slabs)
        AS_STEP("headb.dx1", st, run_split_k(gemm_nn(l1.dz, l1.ldz, l1.wf, H, dxhat, H, R, H, (int)l1.ldz), Lane{st, slab, SLAB_FLOATS, 0}));
    AS_STEP("headb.norm0", st, as_normalize_bwd(dx1_slabs ? slab : dxhat, l1.x, l1.rstd, relu_src, dx, R, H, st, nullptr,
                                                 dx1_slabs ? dx1_slabs : 1, (long)R * H));
    return 0;
}

// The weight gradient of layer i (1, 2) with its bias gradient: dW'[A][N][K] = dz^T . x_hat, db' = column sums of dz
as_wgrad_job wgrad(const HeadStack& s, int i, const float* dz, float* G) {
    const HeadLayer& l = s.l[i];
    as_wgrad_job j{};
    j.g = gemm_tn(dz, l.ldz, l.x, l.ldx, l.dwf, l.K, l.N, l.K, s.R);
    j.g.batch = s.A; j.g.a_batch = l.N; j.g.b_batch = l.x_batch; j.g.c_batch = (long)l.N * l.K;
    j.g.colsum = G + l.b; j.g.colsum_batch = l.N;
    return j;
}
// Layer 1's, whose x_hat all heads share, in its two poses.  transposed (the multi launch): dW1'^T = x_hat^T . dz1 per head
// -- 11 tiles of 128 x 256 like the other layers instead of 22 of 128 x 128 -- stored transposed, the bias gradient being the
// column sums of the B operand.  Plain (the single-problem route): all heads as ONE problem with M = A * 256.
as_wgrad_job wgrad1(const HeadStack& s, float* G, bool transposed) {
    const HeadLayer& l = s.l[0];
    as_wgrad_job j{};
    if (transposed) {
        j.g = gemm_tn(l.x, l.ldx, l.dz, l.ldz, l.dwf, l.K, l.K, l.N, s.R);
        j.g.batch = s.A; j.g.a_batch = l.x_batch; j.g.b_batch = l.N; j.g.c_batch = (long)l.N * l.K;
        j.colsum_b = G + l.b; j.colsum_b_batch = l.N; j.c_trans = 1;
    } else {
        j.g = gemm_tn(l.dz, l.ldz, l.x, l.ldx, l.dwf, l.K, s.A * l.N, l.K, s.R);
        j.g.colsum = G + l.b;
    }
    return j;
}

// Which weight gradients one call computes.  The model's backward issues Layers31Trunk beside the layer-1 recurrence and
// Layer2 beside the layer-0 recurrence: each is one round of <= 192 long-lived workgroups, so that the GRU input-gradient
// GEMM between the two recurrences finds the chip free (a single launch of all four problems kept 184 CUs for ~240 us and
// that GEMM waited for CUs: 113 us instead of 52).
enum class DwPart { All, Layers31Trunk, Layer2 };
// Whose LayerNorm affines a call unfolds (one launch): all three once every dW' is there, i.e. with All or Layer2
enum { UNFOLD_NONE = 0, UNFOLD_L3 = 1, UNFOLD_L2 = 2, UNFOLD_L1 = 4, UNFOLD_ALL = 7 };
// ln: the stream the gradients go to, its slab and CU budget (> 0: beside a recurrence, exact, see gemm_internal.h).  trunk
// (optional): the trunk Linear's weight gradient dzlin^T . y1, which rides in the same launch at N = 2H = 256 (ArtSpeech).
// From 512 rows on several problems go as ONE launch of 128 x 256 tiles + one reduce (as_wgrad_multi); what it declines goes
// to as_gemm_f32 as the same as_gemm plus the two fields the multi launch ignores, slab and CU budget (run_split_k).
int head_bwd_dw(const HeadStack& s, const float* P, float* G, const Lane& ln, DwPart part, int unfold_layers,
                const float* dpre3_in = nullptr, const as_gemm* trunk = nullptr) {
    const hipStream_t st = ln.stream; const int cu_budget = ln.cu_budget;
    const bool multi_ok = s.R % 32 == 0 && s.R >= 512;
    const as_wgrad_job job3 = wgrad(s, 2, dpre3_in ? dpre3_in : s.l[2].dz, G), job2 = wgrad(s, 1, s.l[1].dz, G);
    auto multi = [&](const as_wgrad_job* jobs, int n, const char* phase, int* took) {
        *took = 0;
        if (!multi_ok) return 0;
        AS_PROF(phase, st);
        *took = as_wgrad_multi(jobs, n, ln.slab, ln.slab_floats, cu_budget, st, cu_budget > 0);
        AS_REQUIRE(*took >= 0, *took, "head weight gradients: launch failed");
        return 0;
    };
    int took;
    if (part != DwPart::Layer2) {
        const bool all = part == DwPart::All;
        as_wgrad_job jobs[4] = {job3, wgrad1(s, G, true)};
        int n = 2;
        const bool trunk_rides = trunk && trunk->N == 256;
        if (trunk_rides) jobs[n++].g = *trunk;
        if (all) jobs[n++] = job2;
        AS_TRY(multi(jobs, n, all ? "headb.dw_fused" : "headb.dw31", &took));
        if (!took) {
            AS_STEP("headb.dw3", st, run_split_k(job3.g, ln, cu_budget));
            AS_STEP("headb.dw1", st, run_split_k(wgrad1(s, G, false).g, ln, cu_budget));
            if (all) AS_STEP("headb.dw2", st, run_split_k(job2.g, ln, cu_budget));
        }
        if (trunk && !(took && trunk_rides)) AS_STEP("trunkb.dw", st, run_split_k(*trunk, ln));
    } else {
        AS_TRY(multi(&job2, 1, "headb.dw2", &took));
        if (!took) AS_STEP("headb.dw2", st, run_split_k(job2.g, ln, cu_budget));
    }
    if (unfold_layers == UNFOLD_NONE) return 0;
    const float* dWf[3]; const float* dbf[3]; const float* Wp[3]; const float* gm[3]; const float* bt[3];
    float* dWo[3]; float* dgm[3]; float* dbt[3];
    int Rs[3], Ks[3], cnt = 0;
    for (int i = 2; i >= 0; --i) {
        if (!(unfold_layers & (UNFOLD_L3 << (2 - i)))) continue;
        const HeadLayer& l = s.l[i];
        dWf[cnt] = l.dwf; dbf[cnt] = G + l.b; Wp[cnt] = P + l.w; gm[cnt] = P + l.ln_g; bt[cnt] = P + l.ln_b;
        dWo[cnt] = G + l.w; dgm[cnt] = G + l.ln_g; dbt[cnt] = G + l.ln_b; Rs[cnt] = l.N; Ks[cnt] = l.K; ++cnt;
    }
    AS_STEP("headb.unfold", st, as_unfold3(dWf, dbf, Wp, gm, bt, dWo, dgm, dbt, Rs, Ks, s.A, st, cnt));
    return 0;
}

// ---- per-(device, caller stream) state: a library-owned side stream + fork/join events, and the "head gradients are
// final" event.  Weight-gradient GEMMs (throughput bound, fill the chip) run on the side stream beside the GRU backward
// recurrences (latency bound, 2*B workgroups) instead of after them.  Fork/join are stream-ordered event waits: no host
// synchronisation, capturable in a HIP graph.  Keyed by the CALLER'S stream, so two models (or two host threads) that
// drive the library on different streams of one device never share a side stream or an event; calls on ONE stream are
// ordered by that stream anyway.
struct StreamState {
    int dev = -1; hipStream_t owner = nullptr;
    hipStream_t side = nullptr, side2 = nullptr;   // weight-gradient (and fold) side stream, tail side stream: created on first use with overlap on
    hipEvent_t fold_fork = nullptr, fold_join = nullptr;            // forward: caller -> weight folds -> head GEMM 1
    hipEvent_t fork_trunk = nullptr, fork_dx1 = nullptr, fork_l0 = nullptr;   // backward: behind the trunk's dx, behind dx1, behind the layer-0 recurrence
    hipEvent_t side_to_tail = nullptr, tail_to_caller = nullptr;    // backward joins
    hipEvent_t heads = nullptr;                                     // "head gradients are final": recorded by as_artspeech_bwd
};
int g_overlap = -1;  // -1: not decided yet (environment), 0: off, 1: on
std::mutex g_state_mu;
std::vector<StreamState*> g_states;

StreamState* state_for(hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(g_state_mu);
    for (StreamState* p : g_states)
        if (p->dev == dev && p->owner == st) return p;
    if (g_states.size() >= 256) return nullptr;
    // nothing may be created inside a stream capture: the caller warms the library up once before capturing
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return nullptr;
    StreamState* p = new StreamState;
    p->dev = dev; p->owner = st;
    bool ok = true;
    for (hipEvent_t* e : {&p->heads, &p->fold_fork, &p->fold_join, &p->fork_trunk, &p->fork_dx1, &p->fork_l0, &p->side_to_tail, &p->tail_to_caller})
        ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        delete p;
        return nullptr;
    }
    g_states.push_back(p);
    return p;
}
// the side stream of the caller's stream, or nullptr when overlap is off / unavailable
StreamState* side_for(hipStream_t st) {
    {
        std::lock_guard<std::mutex> lock(g_state_mu);
        if (g_overlap < 0) g_overlap = getenv("ARTSPEECH_NO_OVERLAP") ? 0 : 1;
        if (!g_overlap) return nullptr;
    }
    StreamState* p = state_for(st);
    if (!p) return nullptr;   // no state for this stream (table full, or first call inside a capture): in order on `st`
    {
        std::lock_guard<std::mutex> lock(g_state_mu);
        if (p->side) return p;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return nullptr;
        if (!p->side && hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking) != hipSuccess) {
            p->side = nullptr;
            return nullptr;
        }
        // optional: without it, its work goes to `side`
        if (!p->side2 && hipStreamCreateWithFlags(&p->side2, hipStreamNonBlocking) != hipSuccess) p->side2 = nullptr;
    }
    return p;
}
// The event calls of the schedule: a failure is the HIP error, reported in one form.  join: `to` continues behind what `from` holds
int stream_call(hipError_t e) { AS_REQUIRE(e == hipSuccess, (int)e, "stream fork / join failed: %s", hipGetErrorString(e)); return 0; }
int stream_record(hipEvent_t ev, hipStream_t s) { return stream_call(hipEventRecord(ev, s)); }
int stream_wait(hipStream_t s, hipEvent_t ev) { return stream_call(hipStreamWaitEvent(s, ev, 0)); }
int join(hipStream_t from, hipStream_t to, hipEvent_t ev) { AS_TRY(stream_record(ev, from)); return stream_wait(to, ev); }
// "gradients of the trunk Linear and of all heads are final" -- recorded by as_artspeech_bwd on the stream that produced
// them, so that a data-parallel host can start their all-reduce while the GRU backward is still running.
int record_heads_done(hipStream_t owner, hipStream_t s) {
    StreamState* p = state_for(owner);
    // no per-stream state (more than 256 distinct caller streams, or the first call on a stream inside a capture): the backward
    // then runs in order on the caller's stream and needs no event; as_artspeech_wait_head_grads() reports the missing state itself
    return p ? stream_record(p->heads, s) : 0;
}
// The lanes of one call, resolved once: the caller's stream, the weight-gradient side stream and the tail side stream, each
// with its slab.  The degenerate schedules are states of this value: without a second side stream the tail lane IS the
// weight-gradient lane; flat (sd null: overlap off, no state for the stream, or its first call inside a capture) all three
// are the caller's stream and the main slab, and every fork and join is nothing.
struct Lanes {
    StreamState* sd;   // the events; null: flat
    Lane caller, wgrad, tail;
    // forks are ordinary event records on the caller's stream: while the per-phase timers are on (as_profile_enable: a timing
    // event recorded right behind an event-carrying dispatch reads ~20 us late, which would inflate the phase) and inside a
    // stream capture (graph edges).  Found out only for a call whose forks could ride on a launch (forks_ride: the backward)
    bool plain;
};
Lanes lanes_for(StreamState* sd, hipStream_t st, const HeadStack& hs, bool forks_ride) {
    const Lane caller{st, hs.ws + hs.w.slab, SLAB_FLOATS, 0};
    Lanes ln{sd, caller, caller, caller, true};
    if (!sd) return ln;
    ln.wgrad = Lane{sd->side, hs.ws + hs.w.slab2, SLAB2_FLOATS, 192};
    // second side stream: the small hidden-to-hidden weight gradients (few workgroups, latency bound), so that they run
    // beside the head / input-projection ones instead of queueing behind them: -9 us per step
    ln.tail = sd->side2 ? Lane{sd->side2, hs.ws + hs.w.slab3, SLAB_FLOATS, 192} : ln.wgrad;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (forks_ride) ln.plain = as_profile_active() || hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    return ln;
}
// A fork of the caller's stream behind the launch enqueued while the scope is open.  Unless the lanes are `plain` or the caller
// says the fork cannot ride (something else follows the launch), the event is armed in the stop-event slot and the launch
// carries it on its own dispatch: no marker packet on the critical stream between the launch and what follows it.  to()
// records the event the ordinary way only if no launch took it, then makes the target(s) wait: ONE record on the critical
// stream however many streams fork (every record is a barrier packet there).  seal() ends the riding early, for a fork whose
// to() comes after launches that must not pick the event up.  Flat lanes: nothing happens.  The slot is empty on every way
// out of the scope, an error return included (AsStopEventScope).
struct Fork {
    Fork(const Lanes& ln, hipEvent_t StreamState::*which, bool can_ride = true)
        : from(ln.caller.stream), ev(ln.sd ? ln.sd->*which : nullptr), left(ln.plain || !can_ride ? ev : nullptr), slot(left ? nullptr : ev) {}
    void seal() { if (hipEvent_t e = slot.take()) left = e; }
    int to(hipStream_t a, hipStream_t b = nullptr) {
        if (!ev) return 0;
        seal();
        if (left) AS_TRY(stream_record(ev, from));
        left = nullptr;
        AS_TRY(stream_wait(a, ev));
        return b && b != a ? stream_wait(b, ev) : 0;
    }
    hipStream_t from; hipEvent_t ev, left; AsStopEventScope slot;   // left: still to be recorded (armed: only if no launch takes it)
};

// C = act(A . B^T + bias) on dense operands (an nn.Linear forward: ld = row length)
int linear_fwd(as_gemm g, const float* bias, int act, hipStream_t st) {
    g.bias = bias; g.act = act;
    return as_gemm_f32(&g, st);
}
// the GRU's dW_hh = dgh^T . h_prev with db_hh: B = y shifted by -1 (forward direction) / +1 (reverse) frame inside each
// utterance of T frames; both directions as one batch of two
as_gemm gru_dw_hh(const float* dgh, const float* y, float* dW, float* db, int H, int R, int T) {
    as_gemm g = gemm_tn(dgh, 6 * H, y, 2 * H, dW, H, 3 * H, H, R);
    g.batch = 2; g.a_batch = 3 * H; g.b_batch = H; g.c_batch = 3L * H * H;
    g.b_kshift = -1; g.b_kT = T; g.b_kshift_batch = 2;
    g.colsum = db; g.colsum_batch = 3 * H;
    return g;
}
// What one call of the model works on, and the phases of the step as its members (instead of a dozen parameters each)
struct Step {
    int V, E, H, B, T, R;
    const float* P; const int64_t* tokens; int64_t tok_stride; const int32_t* lengths; float* ws; const as_opts* opts; float pdrop;
    as_layout L; ModelWs w; HeadStack hs;
    int fold_beside(const Lanes& ln) const;
    int gru_trunk_fwd(int train, hipStream_t st) const;
    int simple_trunk_dropout_fwd(hipStream_t st) const, simple_trunk_fwd(hipStream_t st) const;
    int simple_bwd(float* G, const float* dzlin, const float* dpre3, hipStream_t st) const;
    int gru_bwd(float* G, const float* dzlin, const float* dpre3, hipStream_t st) const;
};
int step_of(const as_dims* d, const float* P, const int64_t* tokens, int64_t tok_stride, const int32_t* lengths, int B, int T,
            float* ws, const as_opts* opts, float pdrop, Step* c) {
    *c = Step{d->vocab, d->embed, d->hidden, B, T, B * T, P, tokens, tok_stride, lengths, ws, opts, pdrop, {}, {}, {}};
    AS_TRY(as_artspeech_layout(d, &c->L));
    c->w = model_ws(*d, B, T);
    c->hs = head_stack(*d, c->L, c->R, ws + c->w.head);
    return 0;
}
// The side work of the forward, on the weight-gradient lane: fold the heads' weights and count the bad tokens.  Leaves
// fold_join recorded behind it; the caller's stream waits for that before head GEMM 1.
int Step::fold_beside(const Lanes& ln) const {
    const hipStream_t fs = ln.wgrad.stream;
    const bool late = opts && opts->fold_wait_event;   // a deferred parameter update (as_opts) must land before the folds
    if (late) AS_TRY(stream_wait(fs, (hipEvent_t)opts->fold_wait_event));
    // the folds read the parameters: behind everything the caller's stream holds (the previous optimizer step).  With a
    // deferred update the event above already stands behind that (the update was enqueued after it), and an event record on
    // the caller's stream is a barrier packet in front of the step's first kernel: skipped then
    if (ln.sd && !late) AS_TRY(join(ln.caller.stream, fs, ln.sd->fold_fork));
    AS_TRY(head_fold(hs, P, fs));
    AS_TRY(as_count_bad_tokens(tokens, tok_stride, T, R, V, reinterpret_cast<int*>(ws + w.tokflag), fs));
    return ln.sd ? stream_record(ln.sd->fold_join, fs) : 0;
}
// embedding -> two bidirectional GRU layers -> trunk Linear + ReLU into w.lin
int Step::gru_trunk_fwd(int train, hipStream_t st) const {
    // token table of layer-0 input projections, both directions: [V][2][3H]
    // the step's first kernel, on its critical path: a small dedicated kernel (rowops.hip) while its staging area --
    // (4 E + 64 (E + 1)) floats of dynamic LDS -- stays inside the 64 KB a launch gets without asking (E <= 240)
    if ((long)V * E <= 16384 && ((size_t)4 * E + 64 * ((size_t)E + 1)) * sizeof(float) <= 65536)
        AS_STEP("gru.table0", st, as_token_table(P + L.embedding, P + L.w_ih[0], P + L.b_ih[0], V, 6 * H, E, ws + w.tab0, st));
    else
        AS_STEP("gru.table0", st, linear_fwd(gemm_nt(P + L.embedding, E, P + L.w_ih[0], E, ws + w.tab0, 6 * H, V, 6 * H, E), P + L.b_ih[0], 0, st));
    AS_STEP("gru.fwd_l0", st, as_gru_bidir_fwd_tokens(ws + w.tab0, tokens, tok_stride, V, P + L.w_hh[0], P + L.b_hh[0], lengths, B, T, H, ws + w.y0,
                            train ? ws + w.g0 : nullptr, st));
    const float* l1_in = ws + w.y0;
    if (pdrop > 0.f) {  // nn.GRU inter-layer dropout: layer 1 sees the dropped layer-0 output
        AS_STEP("gru.dropout", st, as_dropout(ws + w.y0, ws + w.y0d, (long)R * 2 * H, pdrop, opts->dropout_seed, st));
        l1_in = ws + w.y0d;
    }
    // input projection of GRU layer 1: [R][2H] . [6H][2H]^T + b.
    // (split arithmetic measured here twice and not kept: the plane-fed kernel of the heads 39.5 vs 43 us + a 10-us plane
    // launch in front of the step's first kernel; both operands split in the kernel, gemm_s6.hip, 35.3 vs 33.1 us alone,
    // tools/bench_linear.py -- at 2.5 GFLOP the launch is bound by its prologue and fill, not by the matrix pipe)
    AS_STEP("gru.xproj1", st, linear_fwd(gemm_nt(l1_in, 2 * H, P + L.w_ih[1], 2 * H, ws + w.xp1, 6 * H, R, 6 * H, 2 * H), P + L.b_ih[1], 0, st));
    AS_STEP("gru.fwd_l1", st, as_gru_bidir_fwd(ws + w.xp1, nullptr, 0, P + L.w_hh[1], P + L.b_hh[1], lengths, B, T, H, ws + w.y1,
                            train ? ws + w.g1 : nullptr, st));
    // (trunk Linear: 10.5 us on the fp32 instruction, 14 - 23 us on either split kernel: 50 - 200 short workgroups)
    AS_STEP("trunk.linear", st, linear_fwd(gemm_nt(ws + w.y1, 2 * H, P + L.lin_w, 2 * H, ws + w.lin, H, R, H, 2 * H), P + L.lin_b, 1, st));
    return 0;
}
// SimpleArtSpeech in training mode (models.py:64,85): Dropout acts on the embedded frame, so every position has its own
// mask and the token-table fold of simple_trunk_fwd does not apply: gather -> counter mask -> Linear + ReLU on all frames
int Step::simple_trunk_dropout_fwd(hipStream_t st) const {
    AS_TRY(as_gather_rows(P + L.embedding, tokens, tok_stride, T, R, E, ws + w.y0, st, V));
    AS_TRY(as_dropout(ws + w.y0, ws + w.y0, (long)R * E, pdrop, opts->dropout_seed, st));
    return linear_fwd(gemm_nt(ws + w.y0, E, P + L.lin_w, E, ws + w.lin, H, R, H, E), P + L.lin_b, 1, st);
}
// SimpleArtSpeech otherwise: relu(Emb Wl^T + bl) per token, gathered by token id
int Step::simple_trunk_fwd(hipStream_t st) const {
    AS_TRY(linear_fwd(gemm_nt(P + L.embedding, E, P + L.lin_w, E, ws + w.tab0, H, V, H, E), P + L.lin_b, 1, st));
    return as_gather_rows(ws + w.tab0, tokens, tok_stride, T, R, H, ws + w.lin, st, V);
}
// ---- backward (behind the heads' input-gradient chain: dzlin = d(trunk pre-activation) [R][H]; dpre3: see head_bwd_dw)
int Step::simple_bwd(float* G, const float* dzlin, const float* dpre3, hipStream_t st) const {
    const Lane me{st, hs.ws + hs.w.slab, SLAB_FLOATS, 0};
    AS_TRY(head_bwd_dw(hs, P, G, me, DwPart::All, UNFOLD_ALL, dpre3));
    AS_TRY(record_heads_done(st, st));
    // The trunk Linear's backward over the rows its forward ran on.  Per frame (dropout): all R frames, then the mask regenerated from
    // the seed and a segmented sum.  Else V token rows: lin = gather(relu(Emb Wl^T + bl)), dzlin carries the ReLU mask: its token sums first
    const bool per_frame = pdrop > 0.f;
    if (!per_frame) AS_TRY(as_token_segsum(dzlin, tokens, tok_stride, T, R, H, V, ws + w.dtab0, st, me.slab, SLAB_FLOATS));
    const float* dz = per_frame ? dzlin : ws + w.dtab0;
    const int rows = per_frame ? R : V;
    as_gemm dw = gemm_tn(dz, H, per_frame ? ws + w.y0 : P + L.embedding, E, G + L.lin_w, E, H, E, rows);
    dw.colsum = G + L.lin_b;
    AS_TRY(run_split_k(dw, me));
    const as_gemm gdx = gemm_nn(dz, H, P + L.lin_w, E, per_frame ? ws + w.dy0 : G + L.embedding, E, rows, E, H);
    AS_TRY(as_gemm_f32(&gdx, st));
    if (!per_frame) return 0;
    AS_TRY(as_dropout(ws + w.dy0, ws + w.dy0, (long)R * E, pdrop, opts->dropout_seed, st));
    return as_token_segsum(ws + w.dy0, tokens, tok_stride, T, R, E, V, G + L.embedding, st, me.slab, SLAB_FLOATS);
}
// The GRU model's backward: the recurrences on the caller's stream, the weight gradients beside them on the weight-gradient lane,
// the small hidden-to-hidden ones and one of the two jobs behind the last recurrence on the tail lane (see lanes_for).
int Step::gru_bwd(float* G, const float* dzlin, const float* dpre3, hipStream_t st) const {
    const Lanes ln = lanes_for(side_for(st), st, hs, true);
    // ---- trunk dx + fork: the head + trunk weight gradients run beside the layer-1 recurrence
    {
        Fork fork(ln, &StreamState::fork_trunk);
        const as_gemm gdx = gemm_nn(dzlin, H, P + L.lin_w, 2 * H, ws + w.dy1, 2 * H, R, 2 * H, H);
        AS_STEP("trunkb.dx", st, as_gemm_f32(&gdx, st));
        AS_TRY(fork.to(ln.wgrad.stream));
    }
    // ---- layer-1 recurrence
    AS_STEP("gru.bwd_l1", st, as_gru_bidir_bwd(ws + w.dy1, ws + w.y1, ws + w.g1, P + L.w_hh[1], lengths, B, T, H, ws + w.dgi1, ws + w.dgh1, st));
    // ---- side work, part 1 (see DwPart): all of it when flat, unless layer 2's is computed later by as_artspeech_dw2()
    as_gemm trunk = gemm_tn(dzlin, H, ws + w.y1, 2 * H, G + L.lin_w, 2 * H, H, 2 * H, R);
    trunk.colsum = G + L.lin_b;
    const bool defer = opts && opts->defer_dw2;
    const bool two_parts = ln.sd != nullptr || defer;
    AS_TRY(head_bwd_dw(hs, P, G, ln.wgrad, two_parts ? DwPart::Layers31Trunk : DwPart::All,
                       defer ? UNFOLD_L3 | UNFOLD_L1 : two_parts ? UNFOLD_NONE : UNFOLD_ALL, dpre3, &trunk));
    // [lin_w, total) of the flat gradient buffer is final from here on ([lin_w, ln2_g) with defer_dw2)
    if (!two_parts || defer) AS_TRY(record_heads_done(st, ln.wgrad.stream));
    // ---- dx1 + fork: the layer-1 weight gradients run beside the layer-0 recurrence.  Input gradient of GRU layer 1:
    // [R][6H] . [6H][2H] (split arithmetic measured slower here, 56 vs 52 us: 200 workgroups x 1.2 MB of weight planes each
    // from L2), then back through the inter-layer dropout: same mask, regenerated from the seed -- the fork cannot ride then
    {
        Fork fork(ln, &StreamState::fork_dx1, !(pdrop > 0.f));
        AS_STEP("grub.dx1", st, run_split_k(gemm_nn(ws + w.dgi1, 6 * H, P + L.w_ih[1], 2 * H, ws + w.dy0, 2 * H, R, 2 * H, 6 * H), ln.caller));
        if (pdrop > 0.f) AS_STEP("gru.dropout", st, as_dropout(ws + w.dy0, ws + w.dy0, (long)R * 2 * H, pdrop, opts->dropout_seed, st));
        AS_TRY(fork.to(ln.wgrad.stream, ln.tail.stream));
    }
    // ---- layer-0 recurrence + fork (the tail's second job; sealed: the side work below is enqueued before the tail forks).
    // Layer 0 sits under the token table: the recurrence keeps per-token sums of its input-side gate gradients in LDS and leaves
    // B tables [V][6H] where dgi0 would have gone (V <= T: they fit): no dgi0, no segmented-sum pass; else dgi0 + as_token_segsum
    const int tok_sums = V <= T && as_gru_bwd_tokens_fits(V, H, T);
    Fork tail_fork(ln, &StreamState::fork_l0);
    if (tok_sums) {
        AS_PROF("gru.bwd_l0", st);
        const int rc = as_gru_bidir_bwd_tokens(ws + w.dy0, ws + w.y0, ws + w.g0, P + L.w_hh[0], lengths, B, T, H, ws + w.dgh0, tokens,
                                               tok_stride, V, ws + w.dgi0, st);
        AS_REQUIRE(rc == 1, rc < 0 ? rc : AS_ERR_UNSUPPORTED, "gru.bwd_l0: launch failed");
    } else {
        AS_STEP("gru.bwd_l0", st, as_gru_bidir_bwd(ws + w.dy0, ws + w.y0, ws + w.g0, P + L.w_hh[0], lengths, B, T, H, ws + w.dgi0, ws + w.dgh0, st));
    }
    tail_fork.seal();
    // ---- side work, part 2
    if (two_parts && !defer) {
        AS_TRY(head_bwd_dw(hs, P, G, ln.wgrad, DwPart::Layer2, UNFOLD_ALL, dpre3));
        AS_TRY(record_heads_done(st, ln.wgrad.stream));  // [lin_w, total) of the flat gradient buffer is final from here on
    }
    as_gemm dw_ih1 = gemm_tn(ws + w.dgi1, 6 * H, pdrop > 0.f ? ws + w.y0d : ws + w.y0, 2 * H, G + L.w_ih[1], 2 * H, 6 * H, 2 * H, R);
    dw_ih1.colsum = G + L.b_ih[1];
    AS_STEP("grub.dw_ih1", ln.wgrad.stream, run_split_k(dw_ih1, ln.wgrad));
    AS_STEP("grub.dw_hh", ln.tail.stream, run_split_k(gru_dw_hh(ws + w.dgh1, ws + w.y1, G + L.w_hh[1], G + L.b_hh[1], H, R, T), ln.tail));
    // ---- tail: the layer-0 gradients.  What follows the last recurrence is the step's tail, and a cross-stream wait costs
    // ~10 us each way on top of the work it guards (measured on the timeline): the LONGER of the two remaining jobs therefore
    // stays on the caller's stream, back to back with the recurrence, and the shorter one forks off.
    //   token sums in the recurrence: hidden-to-hidden GEMM (~30 us) here, table reduction + embedding grads (~13 us) aside;
    //   otherwise: segmented sum + embedding grads (~40 us) here, the GEMM aside.
    const Lane &hh = tok_sums ? ln.caller : ln.tail, &emb = tok_sums ? ln.tail : ln.caller;
    // The weight-gradient lane has its last work of this call queued: the tail lane waits for it HERE, before its own tail work -- a
    // wait that resolves while it idles through the recurrence -- so that the final join is one hop (tail lane -> caller) instead
    // of two (14.6 -> 11 us between the last kernel and Adam).
    if (ln.tail.stream != ln.wgrad.stream) AS_TRY(join(ln.wgrad.stream, ln.tail.stream, ln.sd->side_to_tail));
    AS_TRY(tail_fork.to(ln.tail.stream));
    AS_STEP("grub.dw_hh", hh.stream, run_split_k(gru_dw_hh(ws + w.dgh0, ws + w.y0, G + L.w_hh[0], G + L.b_hh[0], H, R, T), hh));
    // embedding + layer-0 input projection through the token table
    if (tok_sums)
        AS_STEP("grub.segsum", emb.stream, as_sum_partials(ws + w.dgi0, (long)V * 6 * H, B, ws + w.dtab0, emb.stream));
    else
        AS_STEP("grub.segsum", emb.stream, as_token_segsum(ws + w.dgi0, tokens, tok_stride, T, R, 6 * H, V, ws + w.dtab0, emb.stream, emb.slab, SLAB_FLOATS));
    if (E <= 256 && V <= 128 && (6 * H) % 16 == 0) {  // embedding + input-projection gradients of layer 0 from the token sums: one small launch
        AS_STEP("grub.dw_ih0", emb.stream, as_emb_grads(ws + w.dtab0, P + L.embedding, P + L.w_ih[0], V, 6 * H, E, G + L.w_ih[0], G + L.b_ih[0],
                                                  G + L.embedding, emb.stream));
    } else {
        // (only reached on the caller's lane or with the tail lane's slab free: token sums need V <= T, these need V > 128)
        as_gemm dw_ih0 = gemm_tn(ws + w.dtab0, 6 * H, P + L.embedding, E, G + L.w_ih[0], E, 6 * H, E, V);
        dw_ih0.colsum = G + L.b_ih[0];
        AS_STEP("grub.dw_ih0", emb.stream, run_split_k(dw_ih0, emb));
        AS_STEP("grub.demb", emb.stream, run_split_k(gemm_nn(ws + w.dtab0, 6 * H, P + L.w_ih[0], E, G + L.embedding, E, V, E, 6 * H), emb));
    }
    // ---- join: ONE wait on the caller's stream (each costs the tail a few microseconds): the tail lane has waited for the other, or is it
    return ln.sd ? join(ln.tail.stream, st, ln.sd->tail_to_caller) : 0;
}

}  // namespace

extern "C" void as_set_overlap(int32_t on) {
    std::lock_guard<std::mutex> lock(g_state_mu);
    g_overlap = on ? 1 : 0;
}

extern "C" int as_artspeech_wait_head_grads(void* compute_stream, void* waiting_stream) {
    StreamState* p = state_for((hipStream_t)compute_stream);
    AS_REQUIRE(p, AS_ERR_UNSUPPORTED, "as_artspeech_wait_head_grads: as_artspeech_bwd has not run on that stream");
    const hipError_t e = hipStreamWaitEvent((hipStream_t)waiting_stream, p->heads, 0);
    AS_REQUIRE(e == hipSuccess, (int)e, "as_artspeech_wait_head_grads: hipStreamWaitEvent failed: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int as_artspeech_layout(const as_dims* d, as_layout* out) {
    AS_TRY(check_dims(d, "as_artspeech_layout"));
    AS_REQUIRE(out, AS_ERR_BAD_ARG, "as_artspeech_layout: null out");
    const int64_t V = d->vocab, A = d->n_art, E = d->embed, H = d->hidden, N = d->n_samp;
    Carve c;
    as_layout L{};
    L.embedding = c.take(V * E);
    if (!d->simple) {
        const int64_t in[2] = {E, 2 * H};
        for (int l = 0; l < 2; ++l) {
            L.w_ih[l] = c.take(2 * 3 * H * in[l]);
            L.b_ih[l] = c.take(2 * 3 * H);
            L.w_hh[l] = c.take(2 * 3 * H * H);
            L.b_hh[l] = c.take(2 * 3 * H);
        }
        L.lin_w = c.take(H * 2 * H);
    } else {
        for (int l = 0; l < 2; ++l) L.w_ih[l] = L.b_ih[l] = L.w_hh[l] = L.b_hh[l] = -1;
        L.lin_w = c.take(H * E);
    }
    L.lin_b = c.take(H);
    L.ln1_g = c.take(A * H);
    L.ln1_b = c.take(A * H);
    L.w1 = c.take(A * D * H);
    L.b1 = c.take(A * D);
    L.ln3_g = c.take(A * D);
    L.ln3_b = c.take(A * D);
    L.w3 = c.take(A * 2 * N * D);
    L.b3 = c.take(A * 2 * N);
    // last: the group whose gradient a pipelined training loop computes one step late (as_opts.defer_dw2): one
    // contiguous slice [ln2_g, total) for its all-reduce and its Adam update
    L.ln2_g = c.take(A * D);
    L.ln2_b = c.take(A * D);
    L.w2 = c.take(A * D * D);
    L.b2 = c.take(A * D);
    L.total = c.off;
    *out = L;
    return 0;
}

extern "C" int64_t as_head_workspace_floats(const as_dims* d, int64_t rows) {
    if (check_dims(d, "as_head_workspace_floats") != 0 || rows <= 0) return -1;
    return head_ws(*d, rows).total;
}

extern "C" int64_t as_artspeech_workspace_floats(const as_dims* d, int32_t B, int32_t T) {
    if (check_dims(d, "as_artspeech_workspace_floats") != 0 || B <= 0 || T <= 0) return -1;
    return model_ws(*d, B, T).total;
}

extern "C" int as_head_fwd(const as_dims* d, const as_layout* lay, const float* params, const float* x, int64_t rows,
                           float* out, float* ws, int32_t train, void* stream) {
    (void)train;  // the forward keeps its activations in ws either way
    AS_TRY(check_dims(d, "as_head_fwd"));
    AS_REQUIRE(lay && params && x && out && ws && rows > 0 && rows < (1LL << 31), AS_ERR_BAD_ARG, "as_head_fwd: bad argument");
    const HeadStack hs = head_stack(*d, *lay, rows, ws);
    AS_TRY(head_fold(hs, params, (hipStream_t)stream));
    return head_fwd_impl(hs, x, out, (hipStream_t)stream);
}

extern "C" int as_head_bwd(const as_dims* d, const as_layout* lay, const float* params, const float* out, const float* dout,
                           int64_t rows, float* dx, float* grads, float* ws, void* stream) {
    AS_TRY(check_dims(d, "as_head_bwd"));
    AS_REQUIRE(lay && params && out && dout && dx && grads && ws && rows > 0 && rows < (1LL << 31), AS_ERR_BAD_ARG,
               "as_head_bwd: bad argument");
    const HeadStack hs = head_stack(*d, *lay, rows, ws);
    AS_TRY(head_bwd_dx(hs, out, dout, dx, nullptr, (hipStream_t)stream));
    return head_bwd_dw(hs, params, grads, Lane{(hipStream_t)stream, ws + hs.w.slab, SLAB_FLOATS, 0}, DwPart::All, UNFOLD_ALL);
}

extern "C" int as_artspeech_fwd(const as_dims* d, const float* P, const int64_t* tokens, int64_t tok_stride,
                                const int32_t* lengths, int32_t B, int32_t T, float* out, float* ws, int32_t train,
                                const as_opts* opts, void* stream) {
    AS_TRY(check_dims(d, "as_artspeech_fwd"));
    const float pdrop = (opts && train) ? opts->gru_dropout : 0.f;
    AS_REQUIRE(pdrop >= 0.f && pdrop < 1.f, AS_ERR_BAD_ARG, "as_artspeech_fwd: dropout %g not in [0, 1)", (double)pdrop);
    AS_REQUIRE(P && tokens && out && ws && B > 0 && T > 0 && tok_stride >= T, AS_ERR_BAD_ARG, "as_artspeech_fwd: bad argument");
    AS_REQUIRE(d->simple || lengths, AS_ERR_BAD_ARG, "as_artspeech_fwd: lengths required for the GRU model");
    AS_REQUIRE((int64_t)B * T < (1LL << 31), AS_ERR_BAD_ARG, "as_artspeech_fwd: B*T too large");
    hipStream_t st = (hipStream_t)stream;
    Step c;
    AS_TRY(step_of(d, P, tokens, tok_stride, lengths, B, T, ws, opts, pdrop, &c));
    // the weight folds depend on the parameters only: they run on the side stream beside the recurrences
    const Lanes ln = lanes_for(d->simple ? nullptr : side_for(st), st, c.hs, false);
    AS_TRY(c.fold_beside(ln));
    AS_TRY(!d->simple ? c.gru_trunk_fwd(train, st) : pdrop > 0.f ? c.simple_trunk_dropout_fwd(st) : c.simple_trunk_fwd(st));
    if (ln.sd) AS_TRY(stream_wait(st, ln.sd->fold_join));   // folded weights ready before head GEMM 1
    if (!(opts && opts->loss_targets)) return head_fwd_impl(c.hs, ws + c.w.lin, out, st);
    AS_REQUIRE(train && lengths && opts->loss_out && opts->loss_dout && opts->loss_tgt_T >= T, AS_ERR_BAD_ARG,
               "as_artspeech_fwd: fused criterion needs train, lengths, loss_out, loss_dout and loss_tgt_T >= T");
    const Criterion crit{opts->loss_targets, (long)opts->loss_tgt_T, lengths, T, opts->loss_scale, opts->loss_out, opts->loss_dout};
    return head_fwd_impl(c.hs, ws + c.w.lin, out, st, &crit);
}

extern "C" int as_artspeech_dw2(const as_dims* d, const float* P, int32_t B, int32_t T, float* G, float* ws, void* stream) {
    AS_TRY(check_dims(d, "as_artspeech_dw2"));
    AS_REQUIRE(!d->simple && P && G && ws && B > 0 && T > 0, AS_ERR_BAD_ARG, "as_artspeech_dw2: bad argument");
    Step c;
    AS_TRY(step_of(d, P, nullptr, 0, nullptr, B, T, ws, nullptr, 0.f, &c));
    // beside a forward recurrence (2 B workgroups): 192 CUs to count on, and the weight-gradient lane's slab
    return head_bwd_dw(c.hs, P, G, Lane{(hipStream_t)stream, c.hs.ws + c.hs.w.slab2, SLAB2_FLOATS, 192}, DwPart::Layer2, UNFOLD_L2);
}

extern "C" int as_artspeech_bwd(const as_dims* d, const float* P, const int64_t* tokens, int64_t tok_stride,
                                const int32_t* lengths, int32_t B, int32_t T, const float* out, const float* dout, float* G,
                                float* ws, const as_opts* opts, void* stream) {
    AS_TRY(check_dims(d, "as_artspeech_bwd"));
    const float pdrop = opts ? opts->gru_dropout : 0.f;
    AS_REQUIRE(pdrop >= 0.f && pdrop < 1.f, AS_ERR_BAD_ARG, "as_artspeech_bwd: bad dropout option");
    AS_REQUIRE(P && tokens && out && dout && G && ws && B > 0 && T > 0 && tok_stride >= T, AS_ERR_BAD_ARG,
               "as_artspeech_bwd: bad argument");
    AS_REQUIRE(d->simple || lengths, AS_ERR_BAD_ARG, "as_artspeech_bwd: lengths required for the GRU model");
    hipStream_t st = (hipStream_t)stream;
    Step c;
    AS_TRY(step_of(d, P, tokens, tok_stride, lengths, B, T, ws, opts, pdrop, &c));
    float* dzlin = c.hs.ws + c.hs.w.dxhat;  // reused: d(trunk pre-activation) [R][H]
    // heads: input-gradient chain (+ the trunk ReLU mask fused into the last normalize-backward)
    const bool presig = opts && opts->dout_presigmoid;
    AS_TRY(head_bwd_dx(c.hs, out, dout, dzlin, ws + c.w.lin, st, presig));
    AS_REQUIRE(!(d->simple && opts && opts->defer_dw2), AS_ERR_UNSUPPORTED, "as_artspeech_bwd: defer_dw2 is for the GRU model");
    return d->simple ? c.simple_bwd(G, dzlin, presig ? dout : nullptr, st) : c.gru_bwd(G, dzlin, presig ? dout : nullptr, st);
}
