/*
 * artspeech_hip.h -- C ABI of libartspeech_hip.so, the MI355X (gfx950) engine for the
 * phoneme_to_articulation hot path of vribeiro1/artspeech.
 *
 * The reference has no FFI layer: the path sits behind PyTorch module APIs whose device work is
 * implicit (cuDNN GRU / cuBLAS / ATen).  Each entry point below replaces the device work of one of
 * those call sites (cited as file:line relative to the reference root).  Conventions for EVERY call:
 *   - plain pointers and sizes only; pointers are DEVICE pointers unless the name says host;
 *   - the caller owns every buffer (outputs, saved activations, workspaces): nothing is allocated,
 *     freed or synchronised inside; all work is enqueued on `stream` (a hipStream_t passed as void*)
 *     and is re-entrant per stream;
 *   - return value: 0 on success, otherwise a hipError_t (>0) or an AS_ERR_* code (<0);
 *     as_last_error() returns a static message for the last failing call of this thread;
 *   - all floating-point tensors are float32, row-major, contiguous unless a stride is given;
 *     the area function is float64 like the reference.
 */
#ifndef ARTSPEECH_HIP_H
#define ARTSPEECH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AS_ERR_BAD_ARG (-1)      /* null pointer / non-positive size / unsupported combination */
#define AS_ERR_UNSUPPORTED (-2)  /* e.g. a GRU hidden size that is not a multiple of 4 */
#define AS_ERR_WORKSPACE (-3)    /* caller-provided workspace too small */

#define AS_HEAD_HIDDEN 256 /* ArticulatorPredictor's fixed width (encoder_decoder/models.py:12-17) */

const char* as_version(void);    /* "artspeech_hip <semver>" */
const char* as_arch(void);       /* "gfx950" */
const char* as_last_error(void); /* message of the last failing call on this thread ("" if none) */

/* ------------------------------------------------------------------------------------------------
 * Model geometry and the flat parameter layout.
 * All parameters of ArtSpeech / SimpleArtSpeech live in ONE flat float buffer (one gradient buffer,
 * one RCCL all-reduce, one optimizer launch).  as_artspeech_layout() is the single source of truth
 * for where each state_dict tensor of the reference (encoder_decoder/models.py:99-124; key names in
 * SURVEY 8b) sits in that buffer.
 * ---------------------------------------------------------------------------------------------- */
typedef struct as_dims {
    int32_t vocab;   /* V  : nn.Embedding rows                          (models.py:110) */
    int32_t n_art;   /* A  : number of ArticulatorPredictor heads       (models.py:118-120) */
    int32_t embed;   /* E  : embed_dim                                  (models.py:104) */
    int32_t hidden;  /* H  : hidden_size (GRU width, head input width)  (models.py:105) */
    int32_t n_samp;  /* N  : n_samples per contour                      (models.py:106) */
    int32_t simple;  /* 0 = ArtSpeech (BiGRU, models.py:99), 1 = SimpleArtSpeech (models.py:53) */
} as_dims;

/* Offsets (in floats) of every parameter group inside the flat buffer. */
typedef struct as_layout {
    int64_t embedding;  /* [V][E] */
    /* GRU, layer l in {0,1}; forward and reverse direction are ADJACENT (reverse follows forward) so
       that both directions form one stacked matrix: w_ih[l] is [2][3H][I_l], I_0 = E, I_1 = 2H. */
    int64_t w_ih[2], b_ih[2]; /* [2][3H][I_l], [2][3H] */
    int64_t w_hh[2], b_hh[2]; /* [2][3H][H],   [2][3H] */
    int64_t lin_w, lin_b;     /* linear.0: [H][2H] (ArtSpeech) or [H][E] (SimpleArtSpeech), [H] */
    /* heads, stacked over the A predictors (predictors.{a}.*): */
    int64_t ln1_g, ln1_b;     /* linear.0.{weight,bias}  [A][H] */
    int64_t w1, b1;           /* linear.1                [A][256][H], [A][256] */
    int64_t ln2_g, ln2_b;     /* linear.3                [A][256]   -- the group {ln2_g, ln2_b, w2, b2} is the LAST one of */
    int64_t w2, b2;           /* linear.4                [A][256][256], [A][256]   the buffer: [ln2_g, total) (see as_opts) */
    int64_t ln3_g, ln3_b;     /* linear.6                [A][256] */
    int64_t w3, b3;           /* x_coords then y_coords  [A][2][N][256], [A][2][N] */
    int64_t total;            /* number of floats in the flat buffer (multiple of 64) */
} as_layout;

int as_artspeech_layout(const as_dims* dims, as_layout* out);

/* ------------------------------------------------------------------------------------------------
 * Workspace: one caller-allocated float buffer holds every intermediate and saved activation of a
 * training step for a (B, T) batch.  as_artspeech_workspace_floats() returns its size in floats.
 *
 * Token ids: the reference's nn.Embedding (models.py:135) raises IndexError for an id outside [0, V).  The kernels
 * never sync, so instead every kernel that indexes a table by token id clamps the id into the table (no out-of-range
 * access whatever the input), and as_artspeech_fwd leaves the NUMBER of out-of-range ids of its batch in the first
 * 32-bit word of the workspace (int32): the host raises when it reads a non-zero count (the drop-in modules read it
 * after every forward; the training engine whenever it reads the loss).
 * ---------------------------------------------------------------------------------------------- */
int64_t as_artspeech_workspace_floats(const as_dims* dims, int32_t B, int32_t T);

/* Per-call training options (NULL = none).  gru_dropout: nn.GRU's inter-layer dropout (models.py:111; applied
 * to the layer-0 output in training mode only).  The mask is a pure function of (dropout_seed, element): pass the
 * SAME options to the matching as_artspeech_bwd.  Statistical, not bitwise, parity with torch's generator. */
typedef struct as_opts {
    float gru_dropout;      /* 0 <= p < 1: nn.GRU inter-layer dropout (ArtSpeech, models.py:111) or, with dims->simple, the
                               nn.Dropout on the embedded frames of SimpleArtSpeech (models.py:64,85) */
    uint64_t dropout_seed;
    /* as_artspeech_bwd only: non-zero => `dout` already holds the gradient w.r.t. the PRE-sigmoid activations (written by
       as_euclid_masked_fwd_bwd_presigmoid), so the separate dout * out * (1 - out) pass over the contours is skipped. */
    int32_t dout_presigmoid;
    /* Software pipelining of the training loop across the step boundary (ArtSpeech only; artspeech_amd/engine.py):
       as_artspeech_bwd with defer_dw2 != 0 leaves out the weight gradient of the heads' SECOND Linear (9.2 of the step's
       22.9 GFLOP of weight gradients: grads [ln2_g, total) = the LAST group of the flat layout stays unwritten) and
       as_artspeech_dw2() computes it later from the same workspace -- the engine runs it on a side stream beside the NEXT
       step's forward recurrences (64 of 256 CUs busy), followed by that slice's all-reduce and Adam update.
       as_artspeech_fwd with fold_wait_event != NULL (a hipEvent_t) makes the stream that folds the head weights wait for
       that event first (the deferred update must be in place before the heads read their parameters); the recurrences do
       not wait.  The event must stand BEHIND the previous optimizer step on `stream` (the engine enqueues the deferred update
       after a wait for `stream`): the forward then relies on it alone to order its weight folds.  Same arithmetic on the same operands as the unpipelined step: bit-identical parameters. */
    int32_t defer_dw2;
    void* fold_wait_event;
    /* as_artspeech_fwd (training engine): the criterion of train_phoneme_to_articulation.py:86-90 fused into the epilogue of
       the heads' output layer.  loss_targets != NULL (float [B][loss_tgt_T][A][2][N] on the device, loss_tgt_T >= T): the
       forward also writes *loss_out = loss_scale * sum over valid frames of the point distances (loss_scale = 1 / (valid
       frames * A * N); a device scalar) and loss_dout [B][T][A][2][N] = d loss / d(pre-sigmoid activations), which
       as_artspeech_bwd takes as `dout` with dout_presigmoid set -- the separate pass of as_euclid_masked_fwd_bwd_presigmoid
       over the 28 MB of contours and targets disappears.  `out` is written as usual.  Needs 2 N <= 128. */
    const float* loss_targets; int64_t loss_tgt_T; float loss_scale; float* loss_out; float* loss_dout;
} as_opts;

/* ArtSpeech.forward / SimpleArtSpeech.forward (encoder_decoder/models.py:126-145, 75-96).
 *   tokens  : int64 [B][tok_stride] phoneme indices (only the first T columns are read)
 *   lengths : int32 [B] on the DEVICE, sorted descending, 1 <= len <= T, T == max(lengths)
 *             (ignored when dims->simple)
 *   out     : float [B][T][A][2][N]  sigmoid contours
 *   train   : non-zero => keep what as_artspeech_bwd needs in `ws`
 */
int as_artspeech_fwd(const as_dims* dims, const float* params, const int64_t* tokens, int64_t tok_stride,
                     const int32_t* lengths, int32_t B, int32_t T, float* out, float* ws, int32_t train,
                     const as_opts* opts, void* stream);

/* Backward of the above: d(out) -> gradient of EVERY parameter, written (not accumulated) into the
 * flat `grads` buffer (same layout as params).  Must follow as_artspeech_fwd(train=1) on the same ws. */
int as_artspeech_bwd(const as_dims* dims, const float* params, const int64_t* tokens, int64_t tok_stride,
                     const int32_t* lengths, int32_t B, int32_t T, const float* out, const float* dout,
                     float* grads, float* ws, const as_opts* opts, void* stream);

/* The part of the backward that as_artspeech_bwd(opts->defer_dw2) left out: weight / bias gradient of the heads' second Linear
 * and of the LayerNorm in front of it -> grads [ln2_g, total).  Reads what forward + backward left in `ws` (valid until the
 * next as_artspeech_fwd on that workspace reaches its heads, i.e. until that call's fold_wait_event is signalled). */
int as_artspeech_dw2(const as_dims* dims, const float* params, int32_t B, int32_t T, float* grads, float* ws, void* stream);

/* as_artspeech_bwd runs the weight-gradient GEMMs on a library-owned side stream beside the GRU backward
 * recurrences (fork/join by stream-ordered events; `stream` observes completion of everything on return
 * order).  The side stream and its events belong to the (device, `stream`) pair: callers on different streams never
 * share them.  They are created on the first call for that pair, never inside a stream capture (run one step before
 * capturing).  as_set_overlap(0) keeps every kernel on `stream` (default on; env ARTSPEECH_NO_OVERLAP=1 = off). */
void as_set_overlap(int32_t on);

/* Streaming copy dst[i] = src[i] of n floats (n % 4 == 0, 16-byte aligned): a float4 grid-stride kernel.  bench.py times it on
 * 1 GiB to quote the box's measured HBM copy rate (read + write bytes over time) beside the 8 TB/s specification. */
int as_copy_f32(const float* src, float* dst, int64_t n, void* stream);

/* How the library forms fp32 matrix products (every nn.Linear / weight gradient of the path; the reference computes them
 * in fp32: encoder_decoder/models.py:10-33, transformer/models.py:37-100):
 *   0  v_mfma_f32_32x32x2_f32 on the fp32 operands (the exact fp32 matrix instruction);
 *   1  (default) each fp32 operand is split EXACTLY into three bfloat16 numbers (8 + 8 + 8 significand bits) and the
 *      product is rebuilt from six of the nine plane products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- the
 *      three dropped ones are each <= 2^-24 |a||b|.  Inputs, outputs and accumulation stay fp32; against an fp64 product
 *      of the same operands the result is at least as accurate as mode 0 (tests/test_gpu_parity.py::test_split_arith_*).
 *      Kernels without such a path use mode 0.  Inf operands give NaN (inf - inf in the split) where mode 0 gives inf.
 * Process-wide; read at launch time.  Env ARTSPEECH_MATRIX_ARITH=fp32|bf16x6 sets the initial value. */
void as_set_matrix_arith(int32_t mode);
int32_t as_get_matrix_arith(void);

/* The head layers whose reduction is at most 128 deep (Linear 1 at H <= 128, H % 32 == 0; the input gradient of the output layer,
 * "dx3") run, in mode 1 above, on kernels that keep the tile's whole split A operand resident in LDS (csrc/lin_f32.hip).
 * as_set_head_short_k(0) selects the long-reduction kernels that every other head layer uses, for both; the results are the
 * same bit for bit.  Default on.  Process-wide; read at launch time.  For tests and A/B timings. */
void as_set_head_short_k(int32_t on);

/* The criterion fused into the heads' output layer (as_opts.loss_*) reads its targets and writes out and d(out) as 16-byte
 * chunks of whole rows when 2 * n_samples is a multiple of 4 and the three buffers are 16-byte aligned (csrc/lin_f32.hip,
 * criterion_rows_f4).  as_set_lin_out_row_epilogue(0) selects the point-per-lane epilogue that every other case runs; the
 * results are the same bit for bit.  Default on.  Process-wide; read at launch time.  For tests and A/B timings. */
void as_set_lin_out_row_epilogue(int32_t on);

/* Data-parallel hook: make `waiting_stream` wait until the most recent as_artspeech_bwd enqueued on `compute_stream` (same
 * device) has finished the gradients of the trunk Linear and of all heads, i.e. the tail [layout.lin_w, layout.total) of
 * the flat gradient buffer (74 % of the parameters) -- their all-reduce can then run while the GRU backward recurrences
 * are still going. */
int as_artspeech_wait_head_grads(void* compute_stream, void* waiting_stream);

/* ------------------------------------------------------------------------------------------------
 * Building blocks (each is also used by the composite entry points above)
 * ---------------------------------------------------------------------------------------------- */

/* Bidirectional GRU layer recurrence on a packed batch (nn.GRU at encoder_decoder/models.py:111,137;
 * gate order r,z,n; h0 = 0; reverse direction walks t = len_b-1..0; padded outputs are zeros).
 *   gi      : input projections W_ih x + b_ih.  If tokens != NULL it is a TABLE [V][2][3H] indexed by
 *             tokens[b*tok_stride + t] (embedding folded in); else it is [B*T][2][3H].
 *   w_hh    : [2][3H][H], b_hh : [2][3H]
 *   y       : [B][T][2H]  (forward direction in [:H], reverse in [H:])
 *   gates   : NULL (inference) or [B][T][2][4][H] receiving r, z, n, (W_hn h + b_hn) for the backward
 *   H       : 32, 64, 128 run register-resident kernels (W_hh stays in VGPRs for the whole sequence); any other multiple of 4
 *             runs plain kernels that stream W_hh from L2 every step (same results up to the summation order, several
 *             times slower per step) */
int as_gru_bidir_fwd(const float* gi, const int64_t* tokens, int64_t tok_stride, const float* w_hh,
                     const float* b_hh, const int32_t* lengths, int32_t B, int32_t T, int32_t H, float* y,
                     float* gates, void* stream);

/* BPTT of the recurrence.  dy [B][T][2H] -> dgi, dgh [B*T][2][3H] (gradients w.r.t. the input- and
 * hidden-projection pre-activations, zeros at padded frames); weight gradients are time-batched GEMMs
 * over these (done by as_artspeech_bwd). */
int as_gru_bidir_bwd(const float* dy, const float* y, const float* gates, const float* w_hh,
                     const int32_t* lengths, int32_t B, int32_t T, int32_t H, float* dgi, float* dgh,
                     void* stream);

/* Bidirectional LSTM layer, forward / backward (nn.LSTM semantics; the RNNType.LSTM switch of
 * phoneme_to_articulation/__init__.py:47-49 used by principal_components/models/rnn.py:58-68).  Packed-sequence
 * semantics as as_gru_bidir_fwd; gate row order i, f, g, o; h0 = c0 = 0.
 *   H     : 32, 64, 128 run register-resident kernels; any other multiple of 4 (up to 1636 with a backward) the plain
 *           kernels (W_hh streamed from L2 every step; several times slower per step), else AS_ERR_UNSUPPORTED
 *   gi    : W_ih x + b_ih, [B*T][2][4H], or (tokens != NULL) a table [V][2][4H] indexed by tokens[b*tok_stride + t]
 *   w_hh  : [2][4H][H], b_hh : [2][4H];  y : [B][T][2H]
 *   gates : NULL (inference) or [B][T][2][5][H] receiving i, f, g, o, c for the backward
 * Backward: dy [B][T][2H] -> dg [B][T][2][4H], the gradient of the gate pre-activations (input- and hidden-side
 * pre-activations share it; zeros at padded frames); weight gradients are time-batched GEMMs over it. */
int as_lstm_bidir_fwd(const float* gi, const int64_t* tokens, int64_t tok_stride, const float* w_hh, const float* b_hh,
                      const int32_t* lengths, int32_t B, int32_t T, int32_t H, float* y, float* gates, void* stream);
int as_lstm_bidir_bwd(const float* dy, const float* gates, const float* w_hh, const int32_t* lengths, int32_t B, int32_t T,
                      int32_t H, float* dg, void* stream);

/* Strided-batched fp32 GEMM on the f32 MFMA (v_mfma_f32_32x32x2_f32, exact fp32):
 *   C[g][i][j] (+)= act( sum_k Aop[g][i][k] * Bop[g][j][k] + bias[g][j] )
 * Aop[i][k] = A[i*a_i + k*a_k] and Bop[j][k] = B[j*b_j + k*b_k]; one stride of each pair must be 1.
 * act: 0 none, 1 ReLU, 2 sigmoid, 3 exact (erf) GELU.  accumulate != 0 adds to C.  b_kshift/b_kT: if b_kT > 0 the B operand's
 * reduction index k is read at k + b_kshift and is zero unless 0 <= (k % b_kT) + b_kshift < b_kT
 * (the h_{t-1} operand of dW_hh); batch g uses the shift b_kshift + g * b_kshift_batch (forward and reverse direction
 * of a bidirectional layer in one batched call: -1 and +1). */
typedef struct as_gemm {
    const float* A; const float* B; float* C; const float* bias;
    int32_t M, N, K;
    int64_t a_i, a_k, b_j, b_k, ldc;
    int32_t batch; int64_t a_batch, b_batch, c_batch, bias_batch;
    int32_t act, accumulate;
    int32_t b_kshift, b_kT;
    /* optional: workspace enabling deterministic split-K for long reductions with few output tiles
       (weight gradients); optional fused column sums of the A operand, colsum[g][i] = sum_k Aop[g][i][k]
       (bias gradients; needs a_i == 1). */
    float* splitk_ws; int64_t splitk_ws_floats;
    float* colsum; int64_t colsum_batch;
    /* optional GROUPED batches: device arrays of `batch` element offsets that replace g*x_batch for the
       corresponding operand (NULL = linear stride).  Offsets must be multiples of 4 floats.  Used by the
       multi-channel transformer decoder, whose 132 attention blocks per layer read/write irregular
       (channel, head) slices. */
    const int64_t* a_off; const int64_t* b_off; const int64_t* c_off; const int64_t* bias_off;
    /* 0: exact fp32 on the f32 MFMA (default).
       3: the library's current matrix arithmetic (as_set_matrix_arith): in mode 1 the shapes gemm_s6.hip's kernel takes run on
       the bf16 matrix instruction with both operands split exactly into three planes inside the kernel, whatever their size --
       forward (a_k == b_k == 1; plain or relu_bits epilogue), input gradient (a_k == 1, b_j == 1; with res / mask_bits / k_seg)
       and weight gradient (a_i == b_j == 1, >= 256 output tiles of 128 x 128; with colsum); linear or grouped batches,
       K % 16 == 0, float4-clean operands.  Anything else, and mode 0, as 0.  The transformer modules use it for every backward
       GEMM (ARTSPEECH_GRAD_PRECISION, default "lib": 218 -> 187 ms at configs[3]) and offer it for the forward ones
       (ARTSPEECH_GEMM_PRECISION=lib: 173 ms; the full-width contours then sit at 1.19 x the 1e-4 bound against the reference
       fixture, 0.89 x with 0: default 0).  Any other value is refused (AS_ERR_BAD_ARG). */
    int32_t precision;
    int32_t b_kshift_batch;
    /* optional hint for weight-gradient shapes (a_i == b_j == 1 with splitk_ws): the number of CUs the launch can expect to
       have (0 = the whole chip), e.g. 192 while a 64-workgroup recurrence kernel runs beside it on another stream; only the
       split-K factor depends on it, never the result's summation order for a given factor. */
    int32_t cu_budget;
    /* optional extra operands of the general kernel (forward / input-gradient shapes with a reduction-contiguous A; refused
       together with colsum, splitk_ws, accumulate and weight-gradient shapes):
           C = keep ? act(res + acc + bias) : 0
       res       [.][M][N] through (res_ld, res_batch | res_off): the INITIAL VALUE of the accumulators (loaded while the
                 first operand tiles are staged: no extra pass, no epilogue loads); the sum is (res + sum_k in k order) +
                 bias.  In the backward of a ChannelProcessingLayer (transformer/models.py:98) the gradient that arrives
                 over the residual `q + out_proj(ctx)` joins the in-projection's input gradient this way.  Every partial sum
                 carries the residual's magnitude, so the product's rounding error grows with |res| / |sum|: meant for
                 gradients; the forward's residual is added by the LayerNorm that consumes it (as_layernorm_fwd_blockres).
       relu_bits out, with act == 1: one bit per output element, [.][M][ceil(N / 32)] 32-bit words (bit n % 32 of word
                 n / 32 of a row: result > 0), batch stride relu_bits_batch words -- what the backward of the ReLU needs;
       mask_bits in: such a bit image; elements whose bit is clear are stored as 0 (dz = dy * [y > 0], models.py:47-60
                 through autograd): the ReLU backward rides in the epilogue of the GEMM that produces dy, reading 1/32 of
                 what a pass over the saved activations would. */
    const float* res; int64_t res_ld, res_batch; const int64_t* res_off;
    const uint32_t* mask_bits; int64_t mask_batch;
    uint32_t* relu_bits; int64_t relu_bits_batch;
    /* optional SEGMENTED reduction (a_k == 1 input-gradient / forward shapes of the general kernel): the reduction index is
       cut into K / k_seg segments of k_seg (a multiple of 32) and segment s of batch member g reads its A rows from
       A + a_seg_off[g * nseg + s] and its B panel from B + b_seg_off[g * nseg + s] (element offsets, multiples of 4; the
       batch strides / offset tables of A and B are then ignored; inside a segment the ordinary strides apply with k counted
       from the segment's start).  Sums the input gradients of all blocks that read one source channel in ONE GEMM
       (dx[c] = sum_g dz[g] W[g] over the blocks g with src[g] = c) instead of per-block partial tensors + a reduce pass. */
    int32_t k_seg; const int64_t* a_seg_off; const int64_t* b_seg_off;
    /* optional: the A operand is EXACTLY zero below (1: A[i][k] == 0 for k < i) or above (2: for k > i) its diagonal, i and k
       counted in the same index space -- the key-major probabilities P^T[key][q] of a causally masked attention and their
       gradients (transformer/models.py:380-387: both decoder masks are causal).  An output tile then only walks the k-tiles
       in which one of its rows can be non-zero; the skipped products are exact zeros (a non-finite B element in a skipped
       range no longer turns 0 * inf into NaN).  General kernel only, like k_seg; a HINT: operands that are not float4-clean
       (16-byte aligned, strides and contiguous extents multiples of 4) are multiplied over the full range, same result. */
    int32_t k_tri;
} as_gemm;
int as_gemm_f32(const as_gemm* g, void* stream);

/* nn.Linear forward, out[M][N] = act(A[M][K] . W[N][K]^T + bias) (act: 0 none, 1 ReLU, 2 sigmoid; the Linear layers of
 * encoder_decoder/models.py:12-16, 113-116 and transformer/models.py:47-60), in the library's current matrix arithmetic
 * (as_set_matrix_arith): mode 1 emits W as three bfloat16 planes into `planes_ws` (>= as_linear_planes_floats(N, K) floats of
 * scratch, 16-byte aligned) and multiplies on v_mfma_f32_32x32x16_bf16 where the shape allows (K % 32 == 0; N <= 256 or
 * N % 256 == 0; lda % 4 == 0); planes_ws == NULL: both operands are split inside the kernel instead (128 x 128 tiles, K % 16
 * == 0, lda % 4 == 0, ldw % 4 == 0: the form the GRU input projection and the trunk Linear use); everything else -- and mode 0
 * -- runs as_gemm_f32.  tests/ hold both modes' error against an fp64
 * product of the same operands. */
int64_t as_linear_planes_floats(int32_t N, int32_t K);
int as_linear_fwd(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, float* out, int64_t ldo,
                  int32_t M, int32_t N, int32_t K, int32_t act, float* planes_ws, void* stream);

/* ArticulatorPredictor x A + stack + sigmoid (encoder_decoder/models.py:7-33, 141-145) on rows of
 * `x` [rows][in]: out [rows][A][2][N].  Parameters are read from the flat buffer through `lay`.
 * ws: as_head_workspace_floats(). */
int64_t as_head_workspace_floats(const as_dims* dims, int64_t rows);
int as_head_fwd(const as_dims* dims, const as_layout* lay, const float* params, const float* x, int64_t rows,
                float* out, float* ws, int32_t train, void* stream);
/* dout [rows][A][2][N] -> dx [rows][in] and the head parameter gradients inside `grads` (flat). */
int as_head_bwd(const as_dims* dims, const as_layout* lay, const float* params, const float* out,
                const float* dout, int64_t rows, float* dx, float* grads, float* ws, void* stream);

/* EuclideanDistance (phoneme_to_articulation/metrics.py:5-24), reduction "none":
 * out, tgt [frames][A][2][N] -> dist [frames][A][N]. */
int as_euclid_fwd(const float* out, const float* tgt, int64_t frames, int32_t A, int32_t N, float* dist,
                  void* stream);
/* d dist [frames][A][N] -> d out [frames][A][2][N] (NaN where dist == 0, like the reference). */
int as_euclid_bwd(const float* out, const float* tgt, const float* ddist, int64_t frames, int32_t A, int32_t N,
                  float* dout, void* stream);

/* The masked mean of train_phoneme_to_articulation.py:86-90 fused with EuclideanDistance and its
 * gradient: loss = scale * sum_{b, t < len_b} sum_{a,n} dist ; dout = d loss / d out (0 at padded frames).
 * scale = 1 / (N_valid * A * N) with N_valid the GLOBAL number of valid frames (so that DP shards sum
 * to the reference's mean).  out/tgt [B][T or tgt_T][A][2][N]; loss: one float, overwritten;
 * partial: workspace of as_euclid_masked_partials() floats; dout may be NULL (evaluation). */
int32_t as_euclid_masked_partials(void);
int as_euclid_masked_fwd_bwd(const float* out, const float* tgt, int64_t tgt_T, const int32_t* lengths, int32_t B,
                             int32_t T, int32_t A, int32_t N, float scale, float* loss, float* dout,
                             float* partial, void* stream);
/* Same, but `dout` receives d(loss)/d(pre-sigmoid activation) = dout * out * (1 - out): the criterion's backward and the
 * model's final sigmoid backward (models.py:145) in one pass over the contours; pair with as_opts.dout_presigmoid. */
int as_euclid_masked_fwd_bwd_presigmoid(const float* out, const float* tgt, int64_t tgt_T, const int32_t* lengths, int32_t B,
                             int32_t T, int32_t A, int32_t N, float scale, float* loss, float* dout,
                             float* partial, void* stream);

/* MeanP2CPDistance, reduction "none" (phoneme_to_articulation/metrics.py:27-46): for each of `tiles`
 * independent (u, v) pairs: 0.5 * (mean_i min_j |u_i - v_j| + mean_j min_i |u_i - v_j|).
 * Point p of tile t, coordinate c is at u[t*u_tile + p*u_pt + c*u_xy] (same for v): covers both the
 * (*, N, 2) layout the module receives and the (*, 2, N) storage it is a transposed view of.
 * Distances by direct differences (more accurate than torch.cdist's matmul expansion). */
int as_p2cp_fwd(const float* u, int64_t u_tile, int64_t u_pt, int64_t u_xy, int32_t n_u, const float* v,
                int64_t v_tile, int64_t v_pt, int64_t v_xy, int32_t n_v, int64_t tiles, float* out, void* stream);

/* Gradient of as_p2cp_fwd (MeanP2CPDistance, phoneme_to_articulation/metrics.py:27-46, which the reference differentiates
 * through torch.cdist / min): dout [tiles] -> du, dv, addressed like u, v with their own tile / point / xy strides; either may
 * be NULL (that side is not computed; the other side's bits do not change).  With j*(i) the closest v point to u_i, i*(j) the
 * closest u point to v_j -- both from the forward's squared-distance arithmetic, the LOWEST index among equals (torch.min) --
 * and e(a, b) = (a - b) / |a - b|, 0 where |a - b| = 0 (cdist's backward: a coincident pair contributes nothing, no NaN):
 *   du_i = dout * ( e(u_i, v_j*(i)) / (2 n_u) + sum_{j : i*(j) = i} e(u_i, v_j) / (2 n_v) ),  dv_j the mirror image.
 * No atomics, nothing saved by the forward; every sum runs in ascending index order: repeated runs are bit-identical.
 * n_u, n_v in [1, 256], else AS_ERR_UNSUPPORTED before any launch. */
int as_p2cp_bwd(const float* u, int64_t u_tile, int64_t u_pt, int64_t u_xy, int32_t n_u, const float* v, int64_t v_tile,
                int64_t v_pt, int64_t v_xy, int32_t n_v, int64_t tiles, const float* dout, float* du, int64_t du_tile,
                int64_t du_pt, int64_t du_xy, float* dv, int64_t dv_tile, int64_t dv_pt, int64_t dv_xy, void* stream);

/* MeanP2CPDistance (metrics.py:27-46) as the training criterion: the criterion, padding mask and mean of
 * train_phoneme_to_articulation.py:86-90 with the P2CP of every (frame, articulator) contour pair in place of the Euclidean
 * distance, value and gradient from one pass over each tile (the twin of as_euclid_masked_fwd_bwd):
 *   loss = scale * sum_{b, t < len_b, a} p2cp(out[b][t][a], tgt[b][t][a]),   dout [B][T][A][2][N] = d loss / d out.
 * out [B][T][A][2][N], tgt [B][tgt_T][A][2][N] (the (.., 2, N) storage as it is); padded frames are never read (a NaN there
 * does not leak) and their dout is exactly 0; dout may be NULL (evaluation).  scale = 1 / (N_valid * A) with N_valid the
 * GLOBAL number of valid frames, so that data-parallel shards sum to the global mean.  loss: one float, overwritten;
 * partial: workspace of as_p2cp_masked_partials() floats (workgroup sums, then one fixed-order final sum).  N in [1, 256]. */
int32_t as_p2cp_masked_partials(void);
int as_p2cp_masked_fwd_bwd(const float* out, const float* tgt, int64_t tgt_T, const int32_t* lengths, int32_t B, int32_t T,
                           int32_t A, int32_t N, float scale, float* loss, float* dout, float* partial, void* stream);

/* P2CPDistance.forward (encoder_decoder/metrics.py:18-26) reduction: p2cp [B][T][A], lengths ->
 * result[0] = mean_b( mean_{t < len_b, a} p2cp * to_mm ). */
int as_p2cp_utterance_mean(const float* p2cp, const int32_t* lengths, int32_t B, int32_t T, int32_t A, float to_mm,
                           float* result, void* stream);

/* pearsons_correlation (root metrics.py:9-35): Pearson correlation over time of every (utterance, articulator, point)
 * column, x and y planes separately.  out / tgt: [B][T][A][2][N] with element strides out_b / out_t (tgt_b / tgt_t)
 * for the utterance and frame index, the [A][2][N] block of a frame contiguous.  x_corr, y_corr: [B][A][N].
 * corr = sum(vo * vt) / (sqrt(sum vo^2) * sqrt(sum vt^2) + eps); as in the reference the x TARGETS are centred with
 * the x OUTPUTS' mean (metrics.py:22), the y targets with their own (metrics.py:30). */
int as_pearson_fwd(const float* out, int64_t out_b, int64_t out_t, const float* tgt, int64_t tgt_b, int64_t tgt_t,
                   int32_t B, int32_t T, int32_t A, int32_t N, float eps, float* x_corr, float* y_corr, void* stream);

/* Tract variables (tract_variables.py:23-35, 73-125): for each frame and each of n_tv variables the
 * minimum pairwise distance between two point sets and the two closest points (first minimum over
 * arr1 for each arr2 point, then first minimum over arr2).  A set is up to two (channel, start, end)
 * segments of the frame's contours [A][2][N] concatenated.
 *   spec: int32 [n_tv][3 segments][3] = {channel, start, end} for arr1, arr2 part 1, arr2 part 2
 *         (channel < 0 => segment absent), on the DEVICE.
 *   values [frames][n_tv], poc1/poc2 [frames][n_tv][2], idx int32 [frames][n_tv][2] (may be NULL).
 * Limits: N <= 64 points per contour (a lane owns one arr2 point; the reference's slices hold 15 .. 50, n_samples = 50) and
 * a frame [A][2][N] of at most ~15 K floats (it is staged in LDS once): AS_ERR_UNSUPPORTED beyond. */
int as_tract_variables_fwd(const float* contours, int64_t frames, int32_t A, int32_t N, const int32_t* spec,
                           int32_t n_tv, float* values, float* poc1, float* poc2, int32_t* idx, void* stream);

/* area_function (area_function.py:113-142), float64.  Wall point p, coordinate c of frame f is at
 * w[f*frame_stride + p*pt_stride + c*xy_stride].  dists, fx: [frames][n_pts].  dists is the
 * sequential running sum of mid-line segment lengths (same order as the reference's loop).
 * 1 <= n_pts <= 1024 (the reference's air columns hold 100 points per wall). */
int as_area_function_fwd(const double* internal_wall, const double* external_wall, int64_t frame_stride,
                         int64_t pt_stride, int64_t xy_stride, int64_t frames, int32_t n_pts, double alpha,
                         double beta, double* dists, double* fx, void* stream);

/* ---- row operators used by the transformer variant (transformer/models.py) ---------------------------
 * LayerNorm over the last dim (eps 1e-5, biased variance): y = LN(x + res) * gamma + beta.
 * res, gamma/beta (NULL = none / affine-free), xhat and rstd (NULL = not kept) are optional.
 * gamma/beta: group_rows > 0: `group_rows` consecutive rows per parameter set (group g uses gamma + g*D);
 * group_rows < 0: parameter set = row % (-group_rows) (interleaved channels); 0 = one set. */
int as_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* y, float* xhat,
                     float* rstd, int64_t rows, int32_t D, int64_t group_rows, void* stream);

/* Affine-free LayerNorm of x + res where x [channels][rows][per * block] is the concatenation of `per` blocks per channel and
 * res [channels * per][rows][block] is block-major:  xhat[c][r][j*block + f] = LN_row(x[c][r][:] + res[c*per + j][r][f]).
 * This is `LayerNorm(cat_j(q_j + out_proj_j(ctx_j)))` of ChannelInteractionsLayer (transformer/models.py:98, 133-162) with x the
 * out-projections written into the concatenated layout and res the projected queries where the blocks left them: the
 * residual add costs no pass of its own and keeps the reference's order, (sum + bias) + q.  rstd [channels * rows] optional. */
int as_layernorm_fwd_blockres(const float* x, const float* res, float* xhat, float* rstd, int32_t channels, int64_t rows,
                              int32_t per, int32_t block, void* stream);

/* Fold a LayerNorm affine into the following Linear for `heads` independent (W [R][K], gamma/beta [K], b [R])
 * sets: Wf = W.diag(gamma), bf = b + W.beta (then Linear(LN(x)) == x_hat . Wf^T + bf). */
int as_fold_ln(const float* W, const float* gamma, const float* beta, const float* b, float* Wf, float* bf, int32_t heads,
               int32_t R, int32_t K, void* stream);

/* In-place masked softmax over the last dim of scores [Z][Tq][Tk] (nn.MultiheadAttention semantics with float
 * masks): p = softmax(s * scale + attn_mask[b][q][k] + key_padding_mask[b][k]), b = (z / heads) % B.
 * attn_mask / key_padding_mask may be NULL.  A fully masked row gives NaN, as in PyTorch. */
int as_attn_softmax(float* scores, int64_t Z, int32_t Tq, int32_t Tk, int32_t heads, int32_t B, float scale,
                    const float* attn_mask, const float* key_padding_mask, void* stream);

/* Backward of as_attn_softmax, in place on dprobs: dS = P * (dP - sum_k dP * P) * scale. */
int as_attn_softmax_bwd(const float* probs, float* dprobs, int64_t Z, int32_t Tq, int32_t Tk, float scale, void* stream);

/* Fused attention core of nn.MultiheadAttention as used by ChannelProcessingLayer (transformer/models.py:37-100), on already
 * projected tensors:  out[g][b*T + q][h*dh + c] = sum_k softmax_k(Q_h[q] . K_h[k] * scale + attn_mask[b][q][k] + kpm[b][k]) V_h[k][c]
 *   Q, out : [G][B*T][d]     K, V : [G][B*Tk][d]     dh = d / heads in {16, 32, 64}, Tk <= 256 (as_attention_supported)
 *   attn_mask_t      : [B][Tk32][T] additive float mask, KEY-major (the transpose of the reference's (B, T, Tk) mask) with
 *                      the key dimension padded to Tk32 = Tk rounded up to a multiple of 32 (finite padding), or NULL
 *   key_padding_mask : [B][Tk] additive float mask (0 / -inf) or NULL
 *   lse              : optional [G*B*heads][T] log-sum-exp of every score row (what a recomputing backward needs), or NULL
 *   probs_t          : optional [G*B*heads][Tk][Tp] the probabilities, KEY-major, rows padded to Tp = T rounded up to a multiple
 *                      of 32 floats (columns >= T are not written; a 32-query segment of a row is then one 128-byte line)
 *                      (training: as_attention_bwd_ds forms dS^T = P^T o (V dctx^T - D) * scale from it and the grouped GEMMs of
 *                      the backward consume both), or NULL
 *                      (inference: nothing but `out` is written)
 * Scores and probabilities stay in registers (the unfused path writes G*B*heads*T*Tk floats twice).  A fully masked query
 * row yields NaN, as in PyTorch. */
int as_attention_supported(int32_t T, int32_t Tk, int32_t d, int32_t heads);
int as_attention_fwd(const float* Q, const float* K, const float* V, const float* attn_mask_t, const float* key_padding_mask,
                     float* out, float* lse, float* probs_t, int32_t G, int32_t B, int32_t heads, int32_t T, int32_t Tk, int32_t d,
                     float scale, void* stream);
/* The same for a mask the CALLER has checked to be -inf above the diagonal for every utterance (attn_mask[b][q][k] == -inf for
 * k > q: both decoder masks of transformer/models.py:380-387): the key blocks beyond a 32-query strip's own are not computed
 * (their probabilities are exact zeros either way) and the strips are dealt over the waves so that every SIMD gets the same
 * number of blocks.  Identical results. */
int as_attention_fwd_causal(const float* Q, const float* K, const float* V, const float* attn_mask_t, const float* key_padding_mask,
                            float* out, float* lse, float* probs_t, int32_t G, int32_t B, int32_t heads, int32_t T, int32_t Tk,
                            int32_t d, float scale, void* stream);

/* Backward of the attention core, first half, without a dP tensor:  dS^T = P^T o (V dctx^T - D) * scale, that is
 *   ds_t[z][k][q] = probs_t[z][k][q] * (sum_c V_h[k][c] dctx[q][h*dh + c] - D[q]) * scale,   D[q] = sum_c dctx[q][c] ctx[q][c]
 * over the head's dh columns (D = sum_k P dP, without a second pass over the scores).  Shapes as as_attention_fwd; ds_t
 * [G*B*heads][Tk][Tp] is what the two remaining grouped GEMMs (dQ = dS K, dK = dS^T Q) read. */
int as_attention_bwd_ds(const float* V, const float* dctx, const float* ctx, const float* probs_t, float* ds_t, int32_t G, int32_t B,
                        int32_t heads, int32_t T, int32_t Tk, int32_t d, float scale, void* stream);
/* The same when the forward's additive mask was -inf above the diagonal for every utterance (both decoder masks of
 * transformer/models.py:380-387 are causal), i.e. probs_t[z][key][q] == 0 for q < key: only the (32-query strip, 32-key block)
 * pairs on or below the diagonal are computed -- dealt evenly over the workgroup's waves -- the others are stored as zeros.  Same
 * values as as_attention_bwd_ds where P^T is non-zero; exact +0 elsewhere.  T, Tk <= 256 (else the general kernel runs). */
int as_attention_bwd_ds_causal(const float* V, const float* dctx, const float* ctx, const float* probs_t, float* ds_t, int32_t G,
                               int32_t B, int32_t heads, int32_t T, int32_t Tk, int32_t d, float scale, void* stream);

/* dst[c][:] = sum over groups g with src[g] == c of part[g][:] (rows of `len` floats; deterministic order): folds
 * the per-block input gradients of a grouped GEMM back onto the channels the blocks read. */
int as_group_reduce(const float* part, const int32_t* src, int32_t G, int32_t C, int64_t len, float* dst, void* stream);

/* Backward of the affine-free LayerNorm: dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat)), optionally
 * times the ReLU mask (relu_src > 0).  dxhat and dx may alias.  Rows up to 512 wide (wider: D <= 2816). */
int as_layernorm_bwd(const float* dxhat, const float* xhat, const float* rstd, const float* relu_src, float* dx, int64_t rows,
                     int32_t D, void* stream);

/* Backward of as_fold_ln: (dWf, dbf) -> dW = dWf.diag(gamma) + dbf beta^T, dgamma, dbeta (db == dbf). */
int as_unfold_ln(const float* dWf, const float* dbf, const float* W, const float* gamma, const float* beta, float* dW,
                 float* dgamma, float* dbeta, int32_t heads, int32_t R, int32_t K, void* stream);

/* dst[i] = act[i] > 0 ? g[i] : 0 */
int as_relu_bwd(const float* g, const float* act, float* dst, int64_t n, void* stream);

/* out[m][:] = table[tokens[m]][:] + pe[m % T][:]  (Embedding + PositionalEncoding, transformer/models.py:9-34,368-369);
 * table == NULL: out[m][:] += pe[m % T][:] in place. */
int as_embed_posenc(const int64_t* tokens, int64_t tok_stride, const float* table, const float* pe, float* out,
                    int64_t rows, int32_t T, int32_t D, void* stream);

/* dst[i] = a[i] + b[i] (b may be NULL: copy) and dst[i] = a[i] * m[i / row_len] (row mask) */
int as_add(const float* a, const float* b, float* dst, int64_t n, void* stream);
int as_row_scale(const float* a, const float* row_scale, float* dst, int64_t rows, int32_t row_len, void* stream);

/* Inverted dropout with the library's counter-based mask: y[i] = x[i] * keep(seed, i) / (1 - p); x == y allowed.
 * The same (p, seed) regenerates the same mask (that is how the backward works). */
int as_dropout_fwd(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream);

/* evenly_spaced_fx (area_function.py:145-159): resample fx over x (both [frames][n_pts], float64, x increasing) at
 * n_samples evenly spaced abscissae between x[0] and x[-1]; out float32 [frames][2][n_samples] = (abscissae, values),
 * i.e. the reference's vertical-line / polyline intersections = piecewise-linear interpolation. */
int as_evenly_spaced_fx(const double* x, const double* fx, int64_t frames, int32_t n_pts, int32_t n_samples, float* out,
                        void* stream);

/* ---- DeepSpeech2-style articulatory scorer, inference (phoneme_recognition/deepspeech2.py:90-195) -------------
 * Feature maps are channels-last  [B][T][D][32]  (the reference's (B, 32, D, T) permuted (0, 3, 2, 1)).
 * as_conv3x3_stem : nn.Conv2d(Cin, 32, 3, stride 1, padding 1) (:104) of a planar input whose element (b, ci, d, t)
 *                   sits at x[b*sb + ci*sc + d*sd + t*st]; w [9][32][Cin] with tap = kd*3 + kt (the torch weight
 *                   permuted (2, 3, 0, 1)); voicing (NULL or [B][T]) is added to every channel/feature (:175-177).
 * as_conv3x3_c32  : the 32 -> 32 convolutions of ResidualCNN (:22, 25) as an implicit GEMM on the f32 MFMA;
 *                   w [9][32][32]; res (NULL or [B][T][D][32]) is the block's skip input (`out += x`, :46). */
int as_conv3x3_stem(const float* x, int64_t sb, int64_t sc, int64_t sd, int64_t st, const float* w, const float* bias,
                    const float* voicing, float* y, int32_t B, int32_t T, int32_t D, int32_t Cin, void* stream);
int as_conv3x3_c32(const float* x, const float* w, const float* bias, const float* res, float* y, int32_t B, int32_t T,
                   int32_t D, void* stream);

/* ResidualCNN's transpose -> LayerNorm(num_features) -> transpose -> GELU (:30-36, 40-44) on x [rows][D][C]:
 * y[r][d][c] = gelu(LN over d of x[r][:][c], affine gamma[d], beta[d]); eps 1e-5; x == y allowed. */
int as_ln_feat_gelu(const float* x, const float* gamma, const float* beta, float* y, int64_t rows, int32_t D, int32_t C,
                    void* stream);

/* y = gelu(x) (exact erf form, F.gelu default; RecurrentBlock :66); x == y allowed. */
int as_gelu(const float* x, float* y, int64_t n, void* stream);

/* nn.GRU(num_layers=1, bidirectional=False) forward over full-length or ragged rows (RecurrentBlock :54-60, 67), h0 = 0:
 * gi [B][T][3H] = W_ih x + b_ih, w_hh [3H][H], b_hh [3H], y [B][T][H] (zeros at t >= lengths[b]). */
int as_gru_unidir_fwd(const float* gi, const float* w_hh, const float* b_hh, const int32_t* lengths, int32_t B, int32_t T,
                      int32_t H, float* y, void* stream);

/* ---- input gradients of the scorer (DeepSpeech2 above, frozen: no weight gradients).  Feature maps [B][T][D][32]. ----
 * as_gru_unidir_fwd_gates : as_gru_unidir_fwd, also keeping gates [B][T][4][H] = (r, z, n, W_hn h + b_hn) for the backward;
 *                           y is exactly as_gru_unidir_fwd's.
 * as_gru_unidir_bwd       : backward of that recurrence: dy [B][T][H] -> dgi, dgh [B*T][3H], the gradients of W_ih x + b_ih and
 *                           W_hh h + b_hh (gate order r, z, n; zeros at t >= lengths[b]); the input gradient is dgi . W_ih.
 * as_ln_feat_gelu_bwd     : backward of as_ln_feat_gelu: x is the forward's input (mean and rstd are recomputed), dy the
 *                           gradient of its output; dx = d/dx + res (res NULL or [rows][D][C]: a residual gradient fused in).
 * as_conv3x3_stem_bwd     : input gradient of as_conv3x3_stem (w [9][32][Cin], 1 <= Cin <= 4): dy [B][T][D][32] -> dx in the
 *                           forward's planar strides (sb, sc, sd, st); every element of the (B, Cin, D, T) planes is written.
 *                           The 32 -> 32 convolutions need no entry point of their own: their input gradient is
 *                           as_conv3x3_c32 over w'[tap][ci][co] = w[8 - tap][co][ci] with a zero bias.
 * as_gelu_bwd             : dx = dy * gelu'(x) (* scale[i % row_len] if scale: the gamma of an affine LayerNorm before the
 *                           GELU, giving the gradient of its normalised input); dy == dx allowed. */
int as_gru_unidir_fwd_gates(const float* gi, const float* w_hh, const float* b_hh, const int32_t* lengths, int32_t B, int32_t T,
                            int32_t H, float* y, float* gates, void* stream);
int as_gru_unidir_bwd(const float* dy, const float* y, const float* gates, const float* w_hh, const int32_t* lengths, int32_t B,
                      int32_t T, int32_t H, float* dgi, float* dgh, void* stream);
int as_ln_feat_gelu_bwd(const float* x, const float* gamma, const float* beta, const float* dy, const float* res, float* dx,
                        int64_t rows, int32_t D, int32_t C, void* stream);
int as_conv3x3_stem_bwd(const float* dy, const float* w, float* dx, int64_t sb, int64_t sc, int64_t sd, int64_t st, int32_t B,
                        int32_t T, int32_t D, int32_t Cin, void* stream);
int as_gelu_bwd(const float* dy, const float* x, const float* scale, float* dx, int64_t n, int32_t row_len, void* stream);

/* ---- training the scorer (train_phoneme_recognition.py): parameter gradients and the CTC loss ---------------------------
 * Every split reduction below writes at most 256 partial rows to the caller's workspace `ws` (ws_floats floats; too small:
 * AS_ERR_WORKSPACE, whose message names the size needed) and adds them in a fixed order: no atomics, bit-identical repeats.
 * Exact fp32 whatever as_set_matrix_arith says.
 * as_conv3x3_c32_wgrad  : weight and bias gradients of as_conv3x3_c32 (ResidualCNN's cnn1 / cnn2, deepspeech2.py:22, 25):
 *                         dw[tap][co][ci] = sum_{b,t,d} dy[b][t][d][co] * x[b][t+kt-1][d+kd-1][ci] (zero padded, tap = kd*3 + kt,
 *                         the forward's tap layout [9][32][32]), dbias[co] = sum dy; x, dy [B][T][D][32].  Implicit GEMM on the
 *                         f32 MFMA, the positions split over waves.  ws: 256 * (9*1024 + 32) floats suffice.
 * as_conv3x3_stem_wgrad : the same for as_conv3x3_stem (:104): dw [9][32][Cin] (1 <= Cin <= 4), dbias [32]; x is read through the
 *                         forward's planar strides (sb, sc, sd, st); the voicing term has no parameter.  ws: 256 * (288*Cin + 32).
 * as_ln_feat_gelu_param_grad : dgamma[d] = sum_{r,c} dz * xhat, dbeta[d] = sum_{r,c} dz of as_ln_feat_gelu (:31-35, 39-43), where
 *                         dz = dy * gelu'(LN(x)) is the gradient of the LayerNorm's output; mean and rstd are recomputed from
 *                         x [rows][D][C] (C == 32).  ws: 256 * 2 * D.
 * as_layernorm_param_grad : dgamma = sum_r dz * xhat, dbeta = sum_r dz of a row LayerNorm (RecurrentBlock :64, the adapter :75-78)
 *                         from the forward's saved xhat [rows][D] and the gradient dz of its affine output.  ws: 256 * 2 * D. */
int as_conv3x3_c32_wgrad(const float* x, const float* dy, float* dw, float* dbias, int32_t B, int32_t T, int32_t D, float* ws,
                         int64_t ws_floats, void* stream);
int as_conv3x3_stem_wgrad(const float* x, int64_t sb, int64_t sc, int64_t sd, int64_t st, const float* dy, float* dw, float* dbias,
                          int32_t B, int32_t T, int32_t D, int32_t Cin, float* ws, int64_t ws_floats, void* stream);
int as_ln_feat_gelu_param_grad(const float* x, const float* gamma, const float* beta, const float* dy, int64_t rows, int32_t D, int32_t C,
                               float* dgamma, float* dbeta, float* ws, int64_t ws_floats, void* stream);
int as_layernorm_param_grad(const float* dz, const float* xhat, int64_t rows, int32_t D, float* dgamma, float* dbeta, float* ws,
                            int64_t ws_floats, void* stream);

/* torch.nn.CTCLoss (phoneme_recognition/__init__.py:114-120: criterion(log_softmax(outputs).permute(1, 0, 2), targets,
 * input_lengths, target_lengths)).  x: rows of C classes at x[t*sx_t + b*sx_b + c] (the (T, B, C) view of a (B, T, C) tensor costs
 * no copy); logits == 0: x holds log-probabilities, used as given (torch semantics); logits != 0: raw scores, normalised by a
 * log-softmax inside.  targets: int64, padded rows targets[b*tgt_stride + j] (tgt_stride > 0; padding past target_lengths[b]
 * is never read) or torch's concatenated 1-D form (tgt_stride == 0).  input_lengths[b] <= T, target_lengths[b] <=
 * max_target_length <= 2047 (S = 2L + 1 <= 4095 states; AS_ERR_UNSUPPORTED beyond), all int64 on the device; inconsistent
 * lengths give NaN.
 * as_ctc_loss : nll[b] = -log p(target_b | x_b) (inf when no alignment exists), from log-space alpha / beta recursions kept in
 *               ws (with_beta = 0: alpha only -- a loss without gradient); ws: as_ctc_workspace_floats(T, B, max_target_length).
 * as_ctc_grad : from that workspace, grad[t*sg_t + b*sg_b + c] = (exp(lp) - gamma) * scale[b] (scale NULL: 1), gamma the class
 *               occupancy sum_{s: l'_s = c} alpha_t(s) beta_t(s) / (p y_t^c) -- torch's CPU backward with log-probability input,
 *               the gradient with respect to the logits in logits mode.  Zero for t >= input_lengths[b], and for a whole
 *               utterance whose nll is inf when zero_infinity != 0. */
int64_t as_ctc_workspace_floats(int32_t T, int32_t B, int32_t max_target_length);
int as_ctc_loss(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, int32_t logits, const int64_t* targets,
                int64_t tgt_stride, const int64_t* input_lengths, const int64_t* target_lengths, int32_t max_target_length, int32_t blank,
                int32_t with_beta, float* ws, int64_t ws_floats, float* nll, void* stream);
int as_ctc_grad(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, int32_t logits, const int64_t* targets,
                int64_t tgt_stride, const int64_t* input_lengths, const int64_t* target_lengths, int32_t max_target_length, int32_t blank,
                const float* ws, int64_t ws_floats, const float* nll, const float* scale, int32_t zero_infinity, float* grad, int64_t sg_t,
                int64_t sg_b, void* stream);

/* CTC forced alignment (artspeech_amd/csrc/ctc_align.hip): the Viterbi path of the known label sequence through the emissions,
 * expanded into one phoneme token per frame.  It replaces, as a call site, the TextGrid-derived per-frame sequences of
 * generate_vocal_tract_shape_v2.py:135-158 (get_repeated_phoneme / get_phonetic_sequences); the reference has no alignment of its
 * own.  Inputs exactly as as_ctc_loss takes them (x rows, logits, targets padded or concatenated, int64 lengths on the device);
 * max_target_length <= 2047 and T <= 8192, else AS_ERR_UNSUPPORTED before any launch.  State graph and moves are as_ctc_loss's
 * (S = 2L + 1 states; stay, step, skip between different labels; start in state 0 or 1, end in S-1 or S-2), the recursion is
 * max-plus over fp32 log-probabilities, accumulated in fp32 in time order.  Ties: candidates in the order stay, step, skip, a
 * later one wins only if strictly greater; at the end the label state S-2 wins when >= state S-1.  Where the rule of
 * torchaudio.functional.forced_align is well defined these choices coincide with it.
 * For utterance b, Tb = input_lengths[b], L = target_lengths[b]:
 *   score[b]           the path's log-probability; -inf when no alignment exists (Tb < L + adjacent equal labels, a forbidden
 *                      label, Tb == 0 < L); 0 for Tb == 0 == L; NaN for inconsistent lengths.
 *   frame_index[b][t]  the target entry j emitted at frame t < Tb, -1 on a blank frame;  frame_token[b][t]: targets[j] or blank.
 *   frame_filled[b][t] the entry with blanks absorbed: a blank frame belongs to the preceding entry, leading blanks to entry 0;
 *                      -1 with L == 0.
 *   spans[b][j]        (first frame, last frame + 1) of entry j itself;  span_score[b][j]: the mean log-probability of its label
 *                      over those frames.
 * Frames t >= Tb get -1 in the three frame arrays, entries j >= L get (-1, -1) and NaN; an utterance without an alignment gets
 * that fill in all its rows.  Any of the five arrays may be NULL.  The 2-bit back-pointers live in LDS when
 * as_ctc_align_workspace_bytes(...) is 0 (T * (6 + 4 * ceil((2 * max_target_length + 1) / 16)) bytes within 56 KiB), else in ws
 * (that many bytes; too small: AS_ERR_WORKSPACE).  One launch in both input modes, no atomics: repeats are bit-identical. */
int64_t as_ctc_align_workspace_bytes(int32_t T, int32_t B, int32_t max_target_length);
int as_ctc_align(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, int32_t logits, const int64_t* targets,
                 int64_t tgt_stride, const int64_t* input_lengths, const int64_t* target_lengths, int32_t max_target_length, int32_t blank,
                 void* ws, int64_t ws_bytes, float* score, int32_t* frame_index, int32_t* frame_token, int32_t* frame_filled,
                 int32_t* spans, float* span_score, void* stream);

/* CTC beam search over prefixes (artspeech_amd/csrc/ctc_beam.hip): the nbest most probable labellings of every utterance with
 * their scores.  It replaces, as a call site, torchaudio.models.decoder.ctc_decoder(lexicon=None, ...) of
 * test_phoneme_recognition.py:84-91 (flashlight's lexicon-free decoder with a zero language model), with two stated differences:
 * the search starts from "no previous label" (no silence at either end of a result), and identical labellings are merged at the
 * end.  tests/ctc_beam_fp64.py is the contract.  x rows as as_ctc_loss takes them (x[t * sx_t + b * sx_b + c]); input_mode 0:
 * additive scores as given, 1: probabilities (log taken inside, log(0) = -inf), 2: logits (row log-softmax taken inside); NaN
 * counts as -inf.  lengths: int64 on the device, or NULL for T frames each.  Per frame: the beam_size_token classes with the
 * highest x (equal values in ascending class index); every live hypothesis (prefix, ends-in-blank, score) and shortlisted class
 * n contributes score + x[n] (+ sil_score if n == sil; sil = -1: none) to (prefix, blank) / (prefix, label) / (prefix + n,
 * label); contributions below best - beam_threshold are dropped, those with one target merge by max (log_add 0) or logaddexp
 * (1), the beam_size best stay.  Live scores are kept relative to the frame's best, the offset in double.
 *   tokens [B][nbest][T] int32, -1 past a labelling's count;  counts [B][nbest];  scores [B][nbest] float32, -inf where there
 *   is no hypothesis;  num_hyps [B]: min(nbest, live prefixes), 0 when every contribution of some frame was -inf; a length of 0
 *   gives the empty labelling with score 0.
 * Supported: beam_size 1..64, C 2..128, beam_size_token 1..C, T <= 8192, any nbest >= 1; otherwise AS_ERR_UNSUPPORTED before
 * any launch.  ws holds each utterance's prefix trie: as_ctc_beam_workspace_bytes = B * 4 * (N + H) with N = beam_size * T + 1
 * nodes and H = the power of two >= max(64, 2 * N) table entries (0 outside the supported range; host only).  One launch, no
 * float atomics: repeats are bit-identical. */
int64_t as_ctc_beam_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t beam_size);
int as_ctc_beam_search(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, int32_t input_mode,
                       const int64_t* lengths, int32_t blank, int32_t sil, float sil_score, int32_t beam_size, int32_t beam_size_token,
                       float beam_threshold, int32_t log_add, int32_t nbest, int32_t* tokens, int32_t* counts, float* scores,
                       int32_t* num_hyps, void* ws, int64_t ws_bytes, void* stream);

/* ---- evaluating the scorer (test_phoneme_recognition.py): decoding, edit distance, alignment, confusion counts -----------------
 * Integer kernels (artspeech_amd/csrc/recog_eval.hip).  Token batches are int32 rows padded to a pitch (pred [B][P_max],
 * target [B][L_max]) with int32 counts per row (clamped to [0, pitch]; entries past a count are never read).  class_map (int32
 * [n_map], or NULL: identity) is applied to both sides before any comparison -- the reference's _make_tokenized_sequence
 * (phoneme_recognition/__init__.py:435-467) ahead of substitution_matrix; a token outside [0, n_map) gets class -1.
 *
 * as_decode_top1: TopKDecoder.__call__ (decoders.py:36-42) and best-path CTC decoding.  emissions[b*s_b + t*s_t + c], class stride 1
 *   (the (T, B, C) view of a tensor costs no copy); lengths int64 [B] on the device (clamped to [0, T]) or NULL: all T frames.  Per
 *   frame the arg-max class in torch's order (a NaN is the maximum, the lowest index among equals); consecutive repeats of that
 *   raw sequence collapse first, then `blank` is dropped (blank < 0: none), so "a _ a" keeps both a.  tokens [B][T] padded with
 *   -1, counts [B]; argmax (optional, [B][T]): the raw per-frame arg-max, -1 past the length.  T <= 8192 (the row is staged in
 *   LDS), else AS_ERR_UNSUPPORTED before any launch.
 * as_edit_distance: torchmetrics' word_error_rate edit distance (metrics.py:135; insertions, deletions and substitutions cost 1)
 *   of every pair, dist [B] int32; one wave per pair, the table row in registers.  P_max <= 4096, L_max <= 2047, else
 *   AS_ERR_UNSUPPORTED before any launch.
 * as_align_counts: substitution_matrix(..., insertions_and_deletions="both") counts (metrics.py:324-381) over the path of
 *   compute_transitions (:295-321): from the corner, step to the predecessor with the smallest table entry, ties to the diagonal,
 *   then to the previous prediction row, then to the previous target column.  ADDS into counts [(n_classes + 1)][(n_classes + 1)]
 *   int32 (the caller zeroes it; integer atomics, so repeats are bit-identical): a diagonal move, match or not, to [target class]
 *   [predicted class]; a move within one prediction row (a deletion) to [target class][n_classes]; a move within one target
 *   column (an insertion) to [n_classes][predicted class]; a class outside [0, n_classes) takes part in the alignment but is not
 *   counted.  Also writes dist [B].  The uint16 table lives in LDS when as_align_workspace_bytes(...) is 0, else in ws (that many
 *   bytes; too small: AS_ERR_WORKSPACE).  The same size limits as as_edit_distance.
 * as_confusion_counts: the counts of compute_confusion_matrix (__init__.py:410-432): for b < B and t < min(lengths[b], T, S)
 *   (lengths int64 or NULL) ADDS 1 to counts[class(targets[b][t])][class(argmax[b][t])], counts [n][n] int32; frames whose
 *   target or prediction class lies outside [0, n) (the -1 padding) are skipped.  argmax [B][T] (as_decode_top1's), targets [B][S]. */
int as_decode_top1(const float* emissions, int64_t s_b, int64_t s_t, int32_t B, int32_t T, int32_t C, const int64_t* lengths,
                   int32_t blank, int32_t* tokens, int32_t* counts, int32_t* argmax, void* stream);
int as_edit_distance(const int32_t* pred, int32_t P_max, const int32_t* pred_counts, const int32_t* target, int32_t L_max,
                     const int32_t* target_counts, int32_t B, const int32_t* class_map, int32_t n_map, int32_t* dist, void* stream);
int64_t as_align_workspace_bytes(int32_t B, int32_t P_max, int32_t L_max);
int as_align_counts(const int32_t* pred, int32_t P_max, const int32_t* pred_counts, const int32_t* target, int32_t L_max,
                    const int32_t* target_counts, int32_t B, const int32_t* class_map, int32_t n_map, int32_t n_classes, int32_t* counts,
                    int32_t* dist, void* ws, int64_t ws_bytes, void* stream);
int as_confusion_counts(const int32_t* argmax, int32_t T, const int32_t* targets, int32_t S, const int64_t* lengths, int32_t B,
                        const int32_t* class_map, int32_t n_map, int32_t n, int32_t* counts, void* stream);

/* ---- frame-level phoneme classification (artspeech_amd/csrc/frame_ce.hip) ------------------------------------------------
 * The criterion and the ranking metric of the reference's `loss: CE` branch: CrossEntropyLoss.forward (phoneme_recognition/
 * metrics.py:110-120: nn.CrossEntropyLoss over the emission rows that the pad masks keep) and AUROC.__call__ (:189-197:
 * torchmetrics' MulticlassAUROC over the same rows).  Inputs follow as_ctc_loss: rows x[t*sx_t + b*sx_b + c] with class stride
 * 1, int64 targets targets[b*tgt_stride + t] (tgt_stride >= T), int64 lengths [B] on the device (clamped to [0, T]); one target
 * per frame.  A frame (b, t) is valid when t < lengths[b] and its target is not ignore_index.
 * as_frame_ce_loss : per valid frame  (1 - eps) w[y] (-logp_y) + (eps / C) sum_c w[c] (-logp_c),  logp = x - logsumexp(x), w =
 *     weight [C] or 1 (NULL), eps = label_smoothing in [0, 1].  lse [B][T] receives every row's logsumexp (kept for the
 *     backward; frames that are not valid are not written), sums[0] = sum of the frame losses, sums[1] = sum of w[y], both float64:
 *     each frame in float32, the sums in float64 in an order fixed by (T, B) alone -- no float atomics, repeats are bit-identical.
 *     A target outside [0, C) that is not ignore_index never indexes x or weight: it makes sums[0] NaN (and as_frame_ce_grad's
 *     row NaN).  ws: as_frame_ce_workspace_bytes(T, B) bytes (too small: AS_ERR_WORKSPACE); its first 8 bytes are an integer
 *     ticket that must be zero before the first call and that every call leaves zero again -- one call at a time per workspace.
 *     1 <= C <= 4096, else AS_ERR_UNSUPPORTED before any launch.  One launch.
 * as_frame_ce_grad : the gradient with respect to x in the caller's strides, every (t, b, c) written: zero on frames that are
 *     not valid, elsewhere  scale [(1 - eps) w[y] (p_c - [c = y]) + (eps / C) (p_c sum_k w[k] - w[c])],  p_c = exp(x_c - lse);
 *     scale = gout[0] (mean == 0) or gout[0] / sums[1] (mean != 0), both read on the device.  One launch, nothing synchronises.
 * as_frame_auroc : for every class c the one-vs-rest rank statistic over the frames that are valid and whose target lies in
 *     [0, C): n_pos[c] = #{y_i = c}, n_neg[c] = #{y_i != c},  u2[c] = 2 #{(i, j): y_i = c, y_j != c, s_i[c] > s_j[c]} + #{the same
 *     pairs with s_i[c] = s_j[c]}, all int64 [C]; AUROC_c = u2 / (2 n_pos n_neg).  Scores are ranked as given (no softmax inside;
 *     -0 equals +0; finite scores are the contract).  One workgroup per class sorts the class column in LDS: max_frames, the
 *     caller's upper bound on the number of such frames (B * T always is one), may be at most 16384, else AS_ERR_UNSUPPORTED
 *     before any launch -- there is no workspace path; if more frames than max_frames turn out valid the three outputs of every
 *     class are -1 and nothing is written out of bounds.  Integer results: repeats are bit-identical. */
int64_t as_frame_ce_workspace_bytes(int32_t T, int32_t B);
int as_frame_ce_loss(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, const int64_t* targets,
                     int64_t tgt_stride, const int64_t* lengths, const float* weight, int64_t ignore_index, float label_smoothing,
                     float* lse, double* sums, void* ws, int64_t ws_bytes, void* stream);
int as_frame_ce_grad(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, const int64_t* targets,
                     int64_t tgt_stride, const int64_t* lengths, const float* weight, int64_t ignore_index, float label_smoothing,
                     const float* lse, const double* sums, const float* gout, int32_t mean, float* grad, int64_t sg_t, int64_t sg_b,
                     void* stream);
int as_frame_auroc(const float* x, int64_t sx_t, int64_t sx_b, int32_t T, int32_t B, int32_t C, const int64_t* targets,
                   int64_t tgt_stride, const int64_t* lengths, int64_t ignore_index, int32_t max_frames, int64_t* n_pos,
                   int64_t* n_neg, int64_t* u2, void* stream);

/* intersect_semipolar_grid (area_function.py:175-223), float64, batched over frames: air_column [frames][2 walls][2][n_pts]
 * (internal wall first, x row then y row -- the air-column file layout), grid [n_lines][grid_res][2].  For every frame and
 * grid line: flags bit 0 / 1 = the internal / external wall is crossed (0: the reference skips the line), bit 2 = more than
 * 16 crossings of one wall (extra ones dropped); p_int / p_ext [frames][n_lines][2] = the selected point on each wall (the
 * wall's own end point when that wall is not crossed).  Intersections are float64 segment tests ordered along the grid
 * line; the reference computes them with shapely/GEOS (parity unpinned). */
int as_intersect_semipolar_grid(const double* air_column, const double* grid, int64_t frames, int32_t n_pts, int32_t n_lines,
                                int32_t grid_res, int32_t* flags, double* p_int, double* p_ext, void* stream);

/* torch.optim.Adam semantics (L2 weight decay added to the gradient; train_phoneme_to_articulation.py:
 * 177-181) over flat buffers, one launch.  step is the 1-based step count after this update. */
int as_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                 float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                 void* stream);

/* Batched collate on the device (pad_sequence_collate_fn, encoder_decoder/dataset.py:27-65, for a data set that is resident
 * in HBM): utterance b's `lengths[b]` rows start at row `first_row[b]` of `src` ([rows][row_elems], 4-byte floats or 8-byte
 * token ids); out [B][T][row_elems] = those rows followed by `pad_value` (0 for tokens / contours, -1 for voicing). */
int as_gather_pad_rows(const void* src, const int64_t* first_row, const int32_t* lengths, int32_t B, int32_t T,
                       int64_t row_elems, int32_t elem_bytes, double pad_value, void* out, void* stream);

/* All articulator MLPs of a MultiEncoder / MultiDecoder in one launch per direction (principal_components/models/
 * autoencoder.py:153-173 MultiEncoder.forward, :203-213 MultiDecoder.forward; the per-articulator stacks are Encoder / Decoder
 * :83-111, layers = 3: Linear-ReLU-Linear-ReLU-Linear, and PCAEncoder / PCADecoder :10-80, layers = 1: one projection).
 * Group g (sorted-articulator order) maps K_g = dims[2g] inputs through the hidden widths h1, h2 (common to all groups) to
 * N_g = dims[2g + 1] outputs; params[6g + 2l], params[6g + 2l + 1] are the device addresses of W_l [wout][win] (row-major,
 * nn.Linear's layout) and b_l [wout] (0: no bias).  k_max / n_max bound every K_g / N_g.
 *   in_mode 0 (slice):  input_g[r][k] = x[r * x_r + g * x_g + k]                       (the encoder on (rows, A, 2N) targets)
 *   in_mode 1 (gather): input_g[r][k] = in_scale * x[r * x_r + in_idx[g * k_max + k]]  (the decoder on the latent vector;
 *                       in_scale is AutoencoderLoss2's rescale_factor, losses.py:204)
 *   out_mode 0 (stack): y[r * y_r + g * y_g + n] = output_g[r][n]                       (the decoder's torch.concat)
 *   out_mode 1 (max-scatter): y[r * y_r + j] = act(max over the groups g that own j of output_g[r][n], j = out_idx[g * n_max
 *                       + n]), act 0 none / 1 tanh (MultiArticulatorAutoencoder.forward :251); ties go to the first group,
 *                       as torch.max does; an index no group owns is -inf (tanh: -1, zero gradient).  win[r * latent + j]
 *                       records the winning g * n_max + n (-1: none) for the backward.
 * own_ptr [latent + 1] / own (CSR over the latent index j, entries in group order): the (g, n) = g * n_max + n that write j
 * (max-scatter) or the (g, k) = g * k_max + k that read it (gather).  Gather input with max-scatter output is refused.
 * Backward: dy in y's layout (max-scatter: the gradient of the activated latent; y = the forward's output, needed for tanh),
 * dx (optional) in x's layout -- slice: only the slices are written; gather: every j < latent of each row, the readers summed
 * in group order, times in_scale.  dparams (optional; NULL for frozen weights, InputTransform's requires_grad = False,
 * transforms.py:5-14): [groups][as_multi_mlp_param_floats] = per layer W_l [wout_g][win_g] at the start of a slot of
 * [wout_max][win_max], then b_l [wout_max].  Weight gradients are per-row-chunk partials summed in a fixed order; the hidden
 * activations are recomputed from x, nothing is saved between the calls.  Exact fp32 FMA chains, no atomics: bit-identical
 * across runs.  ws: as_multi_mlp_workspace_floats(p, backward) floats.  Limits: every width <= 256 and at most 96 KB of LDS
 * per workgroup for the backward (weights + 32 rows of activations and their gradients): outside them both calls return
 * AS_ERR_UNSUPPORTED before any launch (as_multi_mlp_supported tells in advance). */
typedef struct as_multi_mlp {
    int32_t groups, rows, layers, h1, h2, k_max, n_max, latent;
    const int32_t* dims;
    const int64_t* params;
    int32_t in_mode; float in_scale;
    const float* x; int64_t x_r, x_g;
    const int32_t* in_idx;
    int32_t out_mode, act;
    float* y; int64_t y_r, y_g;
    const int32_t* out_idx;
    const int32_t* own_ptr; const int32_t* own;
    int32_t* win;
    float* ws; int64_t ws_floats;
    const float* dy; float* dx; float* dparams;
} as_multi_mlp;
int32_t as_multi_mlp_supported(int32_t layers, int32_t k_max, int32_t h1, int32_t h2, int32_t n_max);
int64_t as_multi_mlp_param_floats(int32_t layers, int32_t k_max, int32_t h1, int32_t h2, int32_t n_max);
int64_t as_multi_mlp_workspace_floats(const as_multi_mlp* p, int32_t backward);
int as_multi_mlp_fwd(const as_multi_mlp* p, void* stream);
int as_multi_mlp_bwd(const as_multi_mlp* p, void* stream);

/* Incremental PCA of the articulator contours on the device (artspeech_amd/csrc/pca.hip): the fit of
 * train_articulatory_PCA.py:91-108 -- one sklearn.decomposition.IncrementalPCA(n_components = k[a]) per articulator,
 * partial_fit once per loader batch on inputs[:, a, :] -- for all articulators and all batches of a call in one launch sequence:
 * a time-parallel phase (batch means, centred sums of squares and, where the merge is solved on the feature side, the centred
 * cross-products) and ONE launch of a persistent workgroup per articulator that walks the chain of batches.  A partial_fit with n
 * samples seen and m new ones updates mean / variance (Chan), stacks S V (k rows), X - batch_mean (m rows) and the row
 * sqrt(n m / (n + m)) (mean - batch_mean) (the first batch: X - mean only), and keeps the k leading singular values / right
 * singular vectors of the stack, each vector signed so that its largest-magnitude entry is positive (svd_flip,
 * u_based_decision = False).  All arithmetic after the fp32 loads is fp64 (symmetric eigen-solve by cyclic Jacobi with a fixed
 * maximum sweep count); sums have a fixed order: bit-identical repeats.
 *   x      frames, x[row * x_r + a * x_g + f], a < groups, f < features; `rows` rows are consumed in batches of `batch` (the last
 *          may be short), row i of the call being order[i] if order != NULL (int32, the shuffled loader order) else i.
 *   k      device [groups] components per articulator, 1 <= k[a] <= k_max.
 *   n_seen samples seen before this call (0: a fresh fit; the first batch must then hold >= k_max rows).  The fit continues from
 *          `state`, device fp64 [groups][2 features + k_max + k_max features] = mean | variance | singular values | components,
 *          which the call updates: partial_fit is the same call with rows = batch = m.
 *   components [groups][k_max][features], singular_values / explained_variance / explained_variance_ratio [groups][k_max],
 *          noise_variance [groups]: the fp32 results after the last batch (entries >= k[a] are left untouched).
 *   ws     as_pca_workspace_floats(p) floats, 8-byte aligned.
 * Limits: features <= 256, k_max <= min(features, 64): outside them as_pca_fit returns AS_ERR_UNSUPPORTED before any launch
 * (as_pca_supported tells in advance). */
typedef struct as_pca {
    int32_t groups, features, k_max, batch;
    const int32_t* k;
    const float* x; int64_t rows, x_r, x_g;
    const int32_t* order;
    int64_t n_seen;
    double* state;
    float* components; float* singular_values; float* explained_variance; float* explained_variance_ratio; float* noise_variance;
    float* ws; int64_t ws_floats;
} as_pca;
/* the IncrementalPCA(n_components, ...) constructor's and partial_fit's shape checks (train_articulatory_PCA.py:98-101) */
int32_t as_pca_supported(int32_t features, int32_t k_max);
/* scratch of one as_pca_fit call (sklearn allocates its stacked matrix per partial_fit, train_articulatory_PCA.py:108) */
int64_t as_pca_workspace_floats(const as_pca* p);
/* transformers[articulator].partial_fit(inputs[:, i, :]) for every articulator and batch (train_articulatory_PCA.py:104-108) */
int as_pca_fit(const as_pca* p, void* stream);

/* Phoneme-wise mean contour on the device (artspeech_amd/csrc/mean_contour.hip; reference
 * phoneme_to_articulation/phoneme_wise_mean_contour/__init__.py).  Shared layout: `tokens` are int64 ids, a contour row is
 * D = n_articulators * 2 * n_samples floats, and the bank is in CSR form by token: the rows bank_offsets[v] .. bank_offsets[v + 1] - 1
 * of bank_x [M][D] / bank_rel [M] are the stored training frames of token v (bank_offsets int64 [vocab + 1]).
 *
 * as_token_runs: _calculate_tokens_lengths_and_positions (:19-29) and the pos / seq_len of process_sentence_with_pos (:43-47) for
 * every frame of a flat buffer: utterance u holds the rows first_row[u] .. first_row[u] + lengths[u] - 1 (first_row ascending, the
 * HBM-resident data set's layout; a padded (B, T) batch is first_row[b] = b * T).  A run is a maximal stretch of equal consecutive
 * tokens inside one utterance; abs_pos = the frame's index in its run, seq_len = the run's length, rel_pos = abs_pos / seq_len
 * (float32).  Frames outside every utterance (padding) get 0, 0, 0.  A segmented scan over the frames in three launches; ws:
 * as_token_runs_workspace_ints(frames) int32. */
int64_t as_token_runs_workspace_ints(int64_t frames);
int as_token_runs(const int64_t* tokens, const int64_t* first_row, const int32_t* lengths, int32_t utterances, int64_t frames,
                  int32_t* abs_pos, int32_t* seq_len, float* rel_pos, int32_t* ws, void* stream);
/* The per-token mean of forward_mean_contour (:130-137: the mean over the sampled rows of the token), table [vocab][D] float32 from
 * fp64 sums in a fixed order; an empty bank gives a NaN row.  rows != NULL (int64 [M], grouped by token like the bank): the bank is
 * compacted in the same pass, bank_x[k] = src[rows[k]] (src [frames][D]) and bank_rel[k] = src_rel[rows[k]] -- the
 * df[df.token == token].sample(...) of :103 / :130 done once at fit time.  rows == NULL: bank_x is read in place. */
int as_mean_contour_fit(const float* src, const float* src_rel, const int64_t* rows, const int64_t* bank_offsets, int32_t vocab,
                        int32_t D, float* bank_x, float* bank_rel, float* table, void* stream);
/* forward_mean_contour (:125-145) for a padded batch: out [B][T][D] = table[tokens[b][t]] for t < lengths[b], zeros after.  A valid
 * frame whose token lies outside [0, vocab) (NaN) or has an empty bank (the table's NaN row) adds 1 to *flag (device int32). */
int as_mean_contour_fwd(const float* table, const int64_t* bank_offsets, const int64_t* tokens, const int32_t* lengths, int32_t B,
                        int32_t T, int32_t vocab, int32_t D, float* out, int32_t* flag, void* stream);
/* forward_weighted_mean_contour (:86-122) for a padded batch in one launch: for a valid frame q with token v and relative position
 * r = rel_pos[q] (as_token_runs of the batch), out[q] = sum_k w_k bank_x[k] / sum_k w_k over the bank rows k of v with
 * w_k = exp(-|bank_rel[k] - r|) (F.softmin of :107; every exponent lies in [-1, 0]).  The queries of one token inside a chunk of
 * 256 frames share each bank row in tiles of 16; float32 FMAs in a fixed order.  Padded frames give zeros; an empty bank or a token
 * outside [0, vocab) gives NaN and adds to *flag. */
int as_mean_contour_weighted_fwd(const float* bank_x, const float* bank_rel, const int64_t* bank_offsets, const int64_t* tokens,
                                 const float* rel_pos, const int32_t* lengths, int32_t B, int32_t T, int32_t vocab, int32_t D, float* out,
                                 int32_t* flag, void* stream);

/* Masked / weighted MSE with its gradient in one pass (nn.MSELoss(reduction="none") + mask / weights + mean of
 * principal_components/losses.py:215-225 AutoencoderLoss2 and :274-279 RegularizedLatentsMSELoss2):
 *   loss = scale * sum_r w_r sum_f (a[r][f] - b[r][f])^2,   grad[r][f] = 2 * scale * w_r * (a - b)
 * w_r = [r % T < lengths[r / T]] if lengths != NULL (else 1), times row_weights[r] if given.  a, b, grad [rows][feat]
 * contiguous; grad may be NULL; partial: as_masked_mse_partials() floats; the sum is per-workgroup partials, then one fixed-order
 * final sum (deterministic). */
int32_t as_masked_mse_partials(void);
int as_masked_mse_fwd_bwd(const float* a, const float* b, int64_t rows, int64_t feat, const int32_t* lengths, int32_t T,
                          const float* row_weights, float scale, float* loss, float* grad, float* partial, void* stream);

/* Evaluation of the principal-components method on the device (artspeech_amd/csrc/pc_eval.hip; reference
 * phoneme_to_articulation/principal_components/evaluation.py and test_principal_components_autoencoder.py).  Rows are frames:
 * rows = B * T with `lengths` (int32 [B], row b * T + t is valid iff t < lengths[b]; rows % T == 0), every row valid without.
 *
 * as_pc_shapes_eval: one launch for the per-articulator denormalise loops (evaluation.py:373-380,
 * test_principal_components_autoencoder.py:156-160), the upper-incisor injection (evaluation.py:386-400) and the
 * MeanP2CPDistance in mm (test_principal_components_autoencoder.py:166-169).
 *   shapes  [rows][A][2 N]  normalised predictions (the MultiDecoder output);  targets [rows][A][2][N] normalised
 *   mean, std [A][2][N]     the per-articulator Normalize statistics
 *   reference [rows][1][2][N] with ref_idx in [0, A]: copied in at channel ref_idx of both outputs; ref_idx = -1: none
 *   pred_out, tgt_out [rows][A + (ref_idx >= 0)][2][N]: x * std + mean, each operation rounded (bit-equal to the torch expression)
 *   p2cp_mm [rows][A]: the mean point-to-closest-point distance of the denormalised pair (direct differences) times to_mm
 * Each output may be NULL; invalid rows are written as zeros.  One wave per (row, articulator), the tile staged in LDS once.
 * Limit: N <= 128 (AS_ERR_UNSUPPORTED before any launch beyond). */
int as_pc_shapes_eval(const float* shapes, const float* targets, const float* mean, const float* std, const int32_t* lengths,
                      int32_t T, const float* reference, int32_t ref_idx, int64_t rows, int32_t A, int32_t N, float to_mm,
                      float* pred_out, float* tgt_out, float* p2cp_mm, void* stream);
/* Running statistics of a split in device-resident fp64 states that the call updates (no host read per batch); a zero-filled
 * state is the empty one.  Replaces the growing torch.concat + torch.cov of evaluation.py:208-249 and the pandas agg of
 * test_principal_components_autoencoder.py:190-193.
 *   err_state [5][A] = count | mean | M2 (centred sum of squares) | min | max of p2cp_mm [rows][A] over the valid rows
 *   lat_state [1 + L + L L] = count | mean [L] | centred co-moments [L][L] of latents [rows][L] over the valid rows
 * Either half may be absent (p2cp_mm / latents NULL).  A batch is reduced in two passes (mean, then centred sums) and merged by
 * Chan's update; everything after the fp32 loads is fp64, every sum has a fixed order that does not depend on the launch
 * geometry: repeats are bit-identical.  cov = M2 / (n - 1) is torch.cov of the concatenated latents; sqrt(M2 / (n - 1)) is
 * pandas' std.  Limit: L <= 64 (AS_ERR_UNSUPPORTED before any launch beyond). */
int as_pc_eval_accumulate(const float* p2cp_mm, int32_t A, double* err_state, const float* latents, int32_t L, double* lat_state,
                          int64_t rows, const int32_t* lengths, int32_t T, void* stream);

/* Per-segment Pearson correlation of two tables with its summary (artspeech_amd/csrc/report.hip; reference
 * report_phoneme_to_articulation.py:256-285: df.groupby("sentence")[[target, pred]].corr() per tract variable, then mean / std /
 * min / max of the sentences' coefficients).  a, b [rows][K] float32; segment s owns the rows [seg_first[s], seg_first[s + 1])
 * (seg_first int64 [S + 1] on the device, clipped to [0, rows]; segments need not cover all rows).  Every value is (double)x * scale;
 *   corr [S][K]    = sum(ac bc) / sqrt(sum(ac^2) sum(bc^2)) of the centred values; NaN for a segment of fewer than 2 rows and
 *                    whenever the values of either column inside the segment are all bit-identical (pandas answers NaN there; the
 *                    centred sums would be rounding noise)
 *   summary [5][K] = count | mean | std (n - 1) | min | max over the finite corr of each column: std is NaN below 2 finite
 *                    coefficients; without one, count is 0 and the rest NaN.  min and max are elements of corr.
 * One wave per (segment, column), two passes (means, then centred sums), fp64 after the fp32 load, every sum in a fixed order that
 * does not depend on the launch geometry, no atomics: repeats are bit-identical.  S may be 0 (corr may then be NULL). */
int as_segment_corr(const float* a, const float* b, int64_t rows, int32_t K, double scale, const int64_t* seg_first, int32_t S,
                    double* corr, double* summary, void* stream);

/* Contour preparation (artspeech_amd/csrc/contours.hip; reference phoneme_to_articulation/__init__.py:57-118 and
 * phoneme_to_articulation/tail_clipper.py:7-128): tail clipping, upper-incisor frame and optional normalisation of any number of
 * frames in one launch, one wave per (frame, articulator).  All float arrays are float32 and contiguous.
 *   raw  [F][A][N][2]   contour points as the loader yields them (point-major, divided by RES)
 *   refs [F][3][N][2]   TailClipper.TAIL_CLIP_REFERENCES: lower incisor, upper incisor, epiglottis
 *   kinds [A] int32     0 none, 1 tongue, 2 lower lip, 3 upper lip; NULL: no articulator is clipped.  With kinds, N must be 50
 *                       (AS_ERR_UNSUPPORTED before any launch otherwise); without, any N >= 1
 *   thr_*               10/PIXEL_SPACING/RES (tongue, back tail), 5/PIXEL_SPACING/RES (lower lip, front tail), 10/PIXEL_SPACING
 *                       (upper lip, second half), 5/PIXEL_SPACING (upper lip, first half): each computed in double and rounded
 *                       once to float by the caller, which is what torch does with a Python scalar next to a float32 tensor.  The
 *                       upper lip's margins are NOT divided by RES in the reference: on RES-normalised contours they keep every
 *                       point; reproduced as it is
 *   mean, std [A][2][N] optional, together
 *   out [F][A][2][N]    (p[i][c] - u[c]) + 0.3f, u = the last point of the frame's raw upper incisor (two rounded operations);
 *                       with statistics then (. - mean) / std with IEEE division
 *   ref_out [F][1][2][N] optional: the upper incisor in the same frame, never clipped, never normalised
 *   counts [F][A]       optional: points kept before the last resampling; N for an articulator that is not clipped
 *   point_major != 0    out is [F][A][N][2] and holds the clipped points as they are (what the reference's clip_*_tails
 *                       methods return); mean, std and ref_out must be NULL
 * Semantics are the reference's: halves are [:25] and [25:] of the current list, comparisons are strict and in float32 (a point on
 * the threshold is dropped), resampling is F.interpolate(size=50) in nearest mode (output j = kept point floor(j n / 50)).
 * A contour that keeps no point (the reference raises inside F.interpolate; possible for the tongue and the upper lip) gets
 * counts = 0 and a NaN row; every other row is unaffected.  Inputs are finite: the NaN behaviour of argmax is not reproduced. */
int as_prepare_contours(const float* raw, const float* refs, const int32_t* kinds, int64_t F, int32_t A, int32_t N, float thr_tongue,
                        float thr_lower_lip, float thr_upper_lip_front, float thr_upper_lip_back, const float* mean, const float* std,
                        int32_t point_major, float* out, float* ref_out, int32_t* counts, void* stream);
/* Column mean and unbiased standard deviation of x [rows][cols] float32 (the reduction of the reference's
 * scripts/calculate_normalization_statistics.py:73-75): mean [cols], std [cols] float32.  Two passes per partition of
 * AS_COLUMN_STATS_PART_ROWS rows (mean, then centred squares), partitions merged by Chan's update, everything in fp64 after the
 * fp32 load and rounded once at the end; the partition is a constant, the order of every sum is fixed, no atomics: repeats are
 * bit-identical.  rows == 1 gives NaN std, like torch.std.  ws: caller's workspace of at least
 * 2 * ceil(rows / AS_COLUMN_STATS_PART_ROWS) * cols doubles (AS_ERR_WORKSPACE below that). */
#define AS_COLUMN_STATS_PART_ROWS 512
int as_column_mean_std(const float* x, int64_t rows, int32_t cols, float* mean, float* std, double* ws, int64_t ws_doubles,
                       void* stream);

/* Log-mel spectrogram front end of the acoustic recogniser (reference phoneme_recognition/datasets.py:84-92 the transform,
 * :123-132 load_melspec with its mono-to-stereo copy, :47-48 dynamic_range_compression, and the feature part of collate_fn
 * :258-260): torchaudio.transforms.MelSpectrogram's defaults, log(max(., clip)), the channel copy and the padded batch in one
 * launch, from the padded waveforms to the collated tensor.
 *   wave [B] rows of wave_pitch floats, n_samples [B] int64 on the device: utterance b has n_b = n_samples[b] samples
 *   framing             reflect padding by n_fft / 2 on both sides without repeating the edge (index -j reads x[j], index
 *                       n_b - 1 + j reads x[n_b - 1 - j]); frame t covers the padded samples [t hop, t hop + n_fft);
 *                       T_b = 1 + n_b / hop (integer division)
 *   window [n_fft]      the analysis window already centred in the frame
 *   fbanks [n_fft / 2 + 1][n_mels]   mel[m] = sum_k fbanks[k][m] (re^2 + im^2)(X[k]), X the DFT of the windowed frame
 *   clip                > 0: out = log(max(mel, clip)); <= 0: out = mel (power)
 *                       (a NaN sample gives NaN in the frames that read it, as torch.clamp does)
 *   out [B][channels][n_mels][T_max]  the result at t < T_b, bit-identical in every plane; pad_value at T_b <= t < T_max; every
 *                       element is written.  lengths_out [B] int64 (optional) = T_b
 * Supported: n_fft a power of two in [64, 2048], hop >= 1, 1 <= n_mels <= 128, channels 1 or 2, wave_pitch <= 0x3fff0000;
 * AS_ERR_UNSUPPORTED before any launch otherwise.  window and fbanks are 16-byte aligned.  The kernel never reads outside row b: n_b is clamped to [0, wave_pitch], n_b <= n_fft / 2 (where the
 * reflection is undefined; callers refuse it) gives T_b = 0, an all-padding row, and T_b is clamped to T_max.  fp32 throughout,
 * twiddles rounded from fp64; no atomics on global memory: repeats, and a row alone or inside a batch, are bit-identical. */
int as_melspec_fwd(const float* wave, int64_t wave_pitch, const int64_t* n_samples, int32_t B, int32_t n_fft, int32_t hop,
                   const float* window, const float* fbanks, int32_t n_mels, float clip, int32_t channels, float pad_value,
                   float* out, int64_t T_max, int64_t* lengths_out, void* stream);

/* Sample-rate conversion ahead of the log-mel (reference phoneme_recognition/datasets.py:124-126: torchaudio.load, then
 * F.resample(audio, orig_freq, new_freq) when the file's rate is not the model's): the polyphase windowed-sinc resampler of
 * torchaudio's documentation, one launch from a padded batch of rows at the rate `orig` to a padded batch at `new`.
 * With g = gcd(orig, new), o = orig / g input samples step per n = new / g outputs ("phases"), and the dense filter
 * h [n][2 width + o] of the documentation,
 *     y[j n + i] = sum_k h[i][k] xz[j o + k - width],      xz = x inside [0, L) and ZERO outside it (no reflection),
 * cut to M = ceil(n L / o) = (n L + o - 1) / o samples in integers.  The clamp of the filter's argument leaves each phase a
 * band of non-zero taps; the caller hands the band alone:
 *   x [B] rows of x_pitch samples: float32, or (x_int16 != 0) int16 read as value / 32768; n_samples [B] int64 on the
 *                       device: row b has L_b = n_samples[b] samples (clamped to [0, x_pitch]); nothing behind them is read
 *   first [n] int32     tap index k of the first band tap of phase i
 *   coef [band][n]      coef[q][i] = h[i][first[i] + q]: tap-major, so that lanes on adjacent phases read adjacent words
 *   width               the filter's half width in input samples (the k - width above)
 *   lead_min, lead_max  bounds of lead[i] = first[i] - width - floor(i o / n) over the phases: output m = j n + i reads the
 *                       input samples [floor(m o / n) + lead[i], ... + band).  They size the tile's staged span; a first[] that
 *                       breaks them is clamped into the span (wrong values there, never an access outside it)
 *   out [B] rows of out_pitch floats: y at m < M_b, pad_value at M_b <= m < m_max (M_b is clamped to m_max); every element
 *                       of [0, m_max) is written.  lengths_out [B] int64 (optional) = M_b
 * Each output is summed in an order that depends on its phase and the band alone (four interleaved partial sums over q, then
 * (s0 + s1) + (s2 + s3)), never on the batch or the tile; no atomics: repeats, and a row alone or inside a batch, are
 * bit-identical.  as_resample_tile is the host's tile choice: the largest power of two of outputs per workgroup, at most
 * AS_RESAMPLE_MAX_TILE, whose input span as_resample_span(tile, o, n, band, spread = lead_max - lead_min)
 * = floor((tile - 1) o / n) + 2 + spread + band fits AS_RESAMPLE_SPAN_FLOATS floats of LDS; 0 when none does or a limit is broken.
 * Limits: n <= AS_RESAMPLE_MAX_PHASES, band <= AS_RESAMPLE_MAX_BAND, o, x_pitch, out_pitch and m_max <= AS_RESAMPLE_MAX_ROW, B <= 65535;
 * AS_ERR_UNSUPPORTED before any launch beyond them. */
#define AS_RESAMPLE_MAX_PHASES 1024
#define AS_RESAMPLE_MAX_BAND 512
#define AS_RESAMPLE_MAX_ROW 0x3fff0000
#define AS_RESAMPLE_MAX_TILE 1024
#define AS_RESAMPLE_SPAN_FLOATS 12288
int64_t as_resample_span(int64_t tile, int32_t o, int32_t n, int32_t band, int32_t spread);
int32_t as_resample_tile(int32_t o, int32_t n, int32_t band, int32_t spread);
int as_resample_fwd(const void* x, int32_t x_int16, int64_t x_pitch, const int64_t* n_samples, int32_t B, int32_t o, int32_t n,
                    const float* coef, const int32_t* first, int32_t band, int32_t width, int32_t lead_min, int32_t lead_max,
                    float pad_value, float* out, int64_t out_pitch, int64_t m_max, int64_t* lengths_out, void* stream);

/* Contour smoothing: a penalised least-squares B-spline through every contour of a batch, one launch.  The reference smooths
 * each predicted contour with vt_tools.bs_regularization.regularize_Bsplines(contour, 3) before it saves or draws it
 * (generate_vocal_tract_shape_v2.py:173,252; generate_vocal_tract_shape.py:155; phoneme_to_articulation/__init__.py:178-180).
 * vt_tools is not vendored and not pinned by the reference: the definition below is this project's own, an
 * ASSUMPTION whose parity with vt_tools is unpinned.
 * For one contour of N points p_i (float32, widened to float64 once), degree d, K control points:
 *   parameter   s_0 = 0, s_i = s_{i-1} + |p_i - p_{i-1}|; u_i = s_i / s_{N-1}, u_{N-1} = 1 exactly
 *   basis       the clamped uniform knot vector [0]*d + linspace(0, 1, K-d+1) + [1]*d; the span of u is
 *               min(floor(u (K-d)), K-d-1); values by Cox-de Boor
 *   fit         minimise sum_i |S(u_i) - p_i|^2 + lambda sum_j |c_j - 2 c_{j+1} + c_{j+2}|^2, i.e. solve
 *               (B'B + lambda D'D) c = B'p, x and y two right-hand sides of one symmetric positive definite band matrix
 *               (half-bandwidth max(d, 2)), by a square-root-free banded Cholesky factorisation (L diag(d) L')
 *   evaluate    S(v_m), v_m = m / (M-1), m = 0 .. M-1, rounded to float32 once
 * All arithmetic is float64; there is no float32 variant (the matrices reach condition numbers of 1e7).
 *   contours            coordinate xy of point i of contour c at contours[c s_contour + xy s_coord + i s_point] (element strides):
 *                       (B, T, A, 2, N) model outputs and (F, A, N, 2) raw contours both go in as they lie
 *   lengths [B] int64   optional, on the device, with T and A and n_contours = B T A: the contours of frame t >= lengths[b] are
 *                       written as zeros (status 0) and not read
 *   out                 coordinate xy of output m of contour c at out[(2 c + xy) out_pitch + m]; the M outputs of every row
 *                       are written and nothing behind them
 *   status [n_contours] optional int32: bit 0 = zero length (s_{N-1} == 0: every output is p_0, copied bit for bit), bit 1 = a
 *                       non-finite coordinate (this contour's outputs are NaN; no other row is touched by it)
 * Every sum has a fixed order and there are no atomics: two launches give equal bits, and a contour alone or inside a batch
 * gives equal bits.  Limits, refused with AS_ERR_UNSUPPORTED / AS_ERR_BAD_ARG before any launch (never truncated):
 * 1 <= degree <= 3, 2 <= N <= 256, degree + 1 <= K <= 32, 2 <= M <= 1024, lambda > 0 and finite (with lambda = 0 clustered or
 * repeated points leave the matrix singular). */
int as_contour_spline(const float* contours, int64_t s_contour, int64_t s_coord, int64_t s_point, int64_t n_contours, int32_t N,
                      int32_t K, int32_t degree, double lambda, int32_t M, const int64_t* lengths, int32_t T, int32_t A, float* out,
                      int64_t out_pitch, int32_t* status, void* stream);

/* The vocal-tract tube (artspeech_amd/csrc/vocal_tract_tube.hip): the internal and the external wall of every frame, from the
 * frame's articulator contours, in one launch.  The reference calls vt_shape_gen.vocal_tract_tube.generate_vocal_tract_tube at
 * generate_vocal_tract_shape_v2.py:426, generate_vocal_tract_shape.py:34 and scripts/shape_to_air_column.py:77.  vt_shape_gen is
 * neither vendored nor pinned: the definition is THIS PROJECT'S OWN, stated in full at the top of the .hip file, an
 * ASSUMPTION whose parity with vt_shape_gen is unpinned.  In short, per wall and its chain of K contours of N points:
 *   junctions   (i_k, j_k) = the first minimum in row-major order of |c_k[i] - c_{k+1}[j]|^2, float32, dx*dx + dy*dy uncontracted
 *   runs        contour k from its entry (the junction with k-1) to its exit (the junction with k+1); the first and the last
 *               contour start / end at the end that leaves them more points; K = 1: the whole contour
 *   resampling  float64: M points at equal arc-length steps along the concatenated runs, the two ends copied
 *   contours            coordinate xy of point i of articulator a of frame f at contours[f s_frame + a s_art + xy s_coord +
 *                       i s_point] (element strides): (B, T, A, 2, N) model outputs and (F, A, N, 2) raw contours go in as they lie
 *   chains [2][8] int32 ON THE HOST (read before the launch and handed to the kernel by value, so that an index outside [0, A)
 *                       is refused here): row 0 the internal wall's articulator indices, row 1 the external wall's, k_int and
 *                       k_ext of them used; the unused ones are not looked at (-1 by convention)
 *   lengths [B] int64   optional, on the device, with T and frames = B T (frame f = b T + t): a frame t >= lengths[b] gets zeros
 *                       in air, status 0, junctions -1 and length 0, and is not read
 *   air                 coordinate xy of point m of wall w (0 internal, 1 external) of frame f at air[((2 f + w) 2 + xy) ld_out
 *                       + m]: the air-column file layout; the M outputs of every row are written and nothing behind them
 *   status [frames][2]  optional int32: bit 0 = zero length (every output is the first point), bit 1 = a non-finite coordinate
 *                       in a chain contour (this wall's outputs and length are NaN, its junctions -1)
 *   junctions [frames][2][7][2] optional int32: (i_k, j_k), the unused ones -1
 *   wall_length [frames][2]     optional float64: L
 * No atomics, every sum in a fixed order: two launches give equal bits, a frame alone or in a batch gives equal bits.  Limits,
 * refused with AS_ERR_BAD_ARG before any launch (never truncated): 2 <= N <= 128, 1 <= k_int, k_ext <= 8, 2 <= M <= 1024,
 * ld_out >= M, every used chain index in [0, A). */
int as_vocal_tract_tube(const float* contours, int64_t s_frame, int64_t s_art, int64_t s_coord, int64_t s_point, int64_t frames,
                        int32_t A, int32_t N, const int32_t* chains, int32_t k_int, int32_t k_ext, const int64_t* lengths, int32_t T,
                        int32_t M, double* air, int64_t ld_out, int32_t* status, int32_t* junctions, double* wall_length,
                        void* stream);

/* Vocal-tract acoustics (artspeech_amd/csrc/vt_acoustics.hip): the volume-velocity transfer function and the formants of every
 * frame's tube, in one launch.  The reference has no acoustic stage (its area_function.py is imported by nothing): the
 * definition is THIS PROJECT'S OWN, an ASSUMPTION whose parity with any other synthesiser is unpinned.  It has closed-form
 * answers instead: a uniform tube closed at the glottis resonates at (2n - 1) c / 4L.  Lossless walls, float64 throughout:
 *   sections    K per frame, glottis -> lips: area A_i (cm^2) at areas[f a_frame + i a_sec], length l_i (cm) at lengths[f l_frame
 *               + i l_sec] (element strides; l_frame = 0 shares one row of lengths among the frames)
 *   counts [frames] int32, optional, on the device: frame f uses its first counts[f] sections (all K without it; a count above
 *               K reads K)
 *   grid        f_j = f0 + j df, j = 0 .. F-1, f0 > 0, df > 0
 *   chain       k = 2 pi f / c, z_i = rho c / A_i, M_i = [[cos k l_i, j z_i sin k l_i], [j sin(k l_i) / z_i, cos k l_i]],
 *               [[A, B], [C, D]] = M_1 M_2 ... M_K with the glottis on the left
 *   radiation   0: ideal open end, Z = 0.  1: Flanagan's piston in a baffle on the last section, a = sqrt(A_K / pi),
 *               ka = 2 pi f a / c, Z = (rho c / A_K) ((ka)^2 / 2 + j 8 ka / (3 pi))
 *   den, transfer [frames][F] complex128 (real, imaginary; 16-byte aligned): den = C Z + D and H = U_lips / U_glottis = 1 / den
 *   formants    on g = |den|^2.  Coarse minima: bins j in 1 .. F-2 with g_j < g_{j-1} and g_j <= g_{j+1}, in increasing j, the
 *               first n_formants.  Refinement, `rounds` times: the bracket starts as [f_{j-1}, f_{j+1}]; g at lo + (hi - lo) m /
 *               65, m = 1 .. 64; the lowest value wins, among equals the lowest m; the new bracket is that point +- (hi - lo) /
 *               65.  freq [frames][n_formants]: the last bracket's midpoint, i.e. the last winner (f_j when rounds = 0; the
 *               bracket is 2 df (2 / 65)^rounds wide); level: -10 log10 g there, the value that won (g_j when rounds = 0);
 *               found [frames] int32; the slots not found hold NaN
 *   status [frames] int32: bit 0 = some used A_i < min_area (a closure, as in a stop consonant: computed as min_area; not an
 *               error), bit 1 = a non-finite area or length, a length <= 0 or counts[f] < 1 (every output of the frame is NaN,
 *               found = 0; no other frame is touched by it)
 * Every output pointer is optional.  No atomics, every choice in a fixed order: two launches give equal bits, a frame alone or
 * in a batch gives equal bits.  Limits, refused with AS_ERR_BAD_ARG before any launch: 1 <= K <= 1024 (the area function's own),
 * 3 <= F <= 4096, 0 <= n_formants <= 8, 0 <= rounds <= 6, radiation 0 or 1, c, rho, min_area > 0; frames = 0 launches nothing.
 * Left out: wall, viscous and heat losses, formant bandwidths, a nasal branch, a time-domain waveform. */
int as_vt_acoustics(const double* areas, int64_t a_frame, int64_t a_sec, const double* lengths, int64_t l_frame, int64_t l_sec,
                    const int32_t* counts, int64_t frames, int32_t K, double f0, double df, int32_t F, int32_t radiation, double c,
                    double rho, double min_area, int32_t n_formants, int32_t rounds, double* den, double* transfer, double* freq,
                    double* level, int32_t* found, int32_t* status, void* stream);

/* Speech from the tube (artspeech_amd/csrc/vt_synth.hip): a glottal source and a time-domain Kelly-Lochbaum waveguide whose
 * sections vary in time.  The reference has no acoustic stage: the definition is THIS PROJECT'S OWN, an ASSUMPTION whose parity
 * with any other synthesiser is unpinned.  Its closed forms: a uniform ladder of K sections resonates at (2n - 1) fs / 4K, and
 * a static ladder's impulse response is the direct solve of its 2K steady-state equations.  All arithmetic and state: float64.
 * Conventions of both entry points:
 *   B utterances of T frame slots, (B, T) arrays contiguous; frames [B] int32 on the device, read into [0, T]: utterance b uses
 *   frames[b] frames.  S >= 1 samples per frame: frame t sits at sample t S, utterance b has n_b = frames[b] S samples, and the
 *   sample rate is fs = S x the frame rate.  A per-frame control x is read at sample n as x[n] = x_t + (x_t' - x_t) (s / S),
 *   t = n div S, s = n mod S, t' = min(t + 1, frames[b] - 1): the last frame is held.  Output rows have a pitch >= T S; the
 *   samples n_b .. pitch - 1 are written as 0 and nothing behind the pitch is written.  T S < 2^31, S <= 2^24.
 *   noise       nu(seed, stream, b, n): idx = ((2 b + stream) << 40) | n, z = seed + (idx + 1) 0x9E3779B97F4A7C15 mod 2^64,
 *               z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9, z = (z ^ (z >> 27)) 0x94D049BB133111EB, z ^= z >> 31 (the splitmix64
 *               finaliser of as_dropout_fwd), u = (z >> 11) 2^-53, nu = 2 u - 1 in [-1, 1): exact in float64.  Stream 0 is
 *               aspiration, stream 1 frication.
 * as_vt_glottal_source: f0 (Hz), voiced_amp, asp_amp (B, T) float64 -> source (B, pitch) float64.
 *   phase       g_t = max(f0_t, 0) per frame, g[n] interpolated as above (so g[n] = max(g[n], 0): never negative);
 *               phase[n] = sum_{m < n} g[m] / fs, evaluated as base_t + (g_t s + (g_t' - g_t) (s (s - 1) / 2) / S) / fs with
 *               base_t = sum_{u < t} (g_u S + (g_u' - g_u) (S - 1) / 2) / fs: a scan over frames and a closed form per sample
 *   pulse       theta = phase - floor(phase); Rosenberg: theta < rise: (1 - cos(pi theta / rise)) / 2; rise <= theta < rise +
 *               fall: cos(pi (theta - rise) / (2 fall)); otherwise 0.  Continuous everywhere, the wrap included.
 *   source[n] = voiced_amp[n] pulse(theta) + asp_amp[n] nu(seed, 0, b, n)
 *   status [B]  optional int32: bit 1 = a non-finite f0, voiced_amp or asp_amp in a used frame: the row's n_b samples are NaN
 *               and no other row is touched.  rise, fall > 0, rise + fall <= 1 (defaults of the package: 0.40, 0.16).
 * as_vt_waveguide: section 0 is the glottis, K_b - 1 the lips; every section is c / fs long, one sample of delay each way (the
 * length appears nowhere else).
 *   areas       A (cm^2) of section j of frame t of utterance b at areas[b a_utt + t a_frame + j a_sec] (element strides),
 *               rows of Kmax sections; sections [B] int32 on the device: K_b in [1, min(64, Kmax)]
 *   per frame   A = max(A, min_area), k_j = (A_j - A_{j+1}) / (A_j + A_{j+1}), j = 0 .. K-2.  The reflection coefficients, not
 *               the areas, are interpolated per sample (a convex combination keeps |k| < 1 and the division off the sample path)
 *   state       right-going R_i and left-going L_i pressure waves, zero at n = 0.  Per sample, the right-hand sides from the
 *               state before:   y = (1 + r_l) R_{K-1};  out[n] = y - y_prev (radiation 1, "difference"; y_prev = 0 at n = 0)
 *               or y (radiation 0, "none");
 *                 w_j      = k_j[n] (R_j - L_{j+1})                 j = 0 .. K-2
 *                 R'_{j+1} = mu ((R_j + w_j) + e_{j+1}[n])
 *                 L'_j     = mu (L_{j+1} + w_j)
 *                 R'_0     = mu (source[n] + r_g L_0)
 *                 L'_{K-1} = mu (r_l R_{K-1})
 *   frication   inject_section (B, T) int32 and inject_gain (B, T) float64, both or neither: e_i[n] = inject_gain[n] nu(seed,
 *               1, b, n) when i == inject_section[t] and 0 otherwise; the section is constant over a frame (-1: none, and the
 *               gain is not multiplied in), the gain is interpolated
 *   out64 (B, pitch) float64, out32 (B, pitch) float32 = out64 rounded; either may be NULL
 *   status [B]  optional int32: bit 0 = some used area below min_area, computed as min_area (a closure, not an error); bit 1 =
 *               a non-finite or non-positive area, or a non-finite source sample or gain, in a used frame: that utterance's
 *               n_b samples are NaN and no other utterance is touched
 * Refused before any launch, never truncated: K_b outside [1, 64] (AS_ERR_UNSUPPORTED); K_b > Kmax, an inject_section of a used
 * frame outside {-1} and [1, K_b - 1], a pitch below T S (AS_ERR_BAD_ARG).  To refuse, as_vt_waveguide reads sections, frames
 * and inject_section back and waits for `stream` once before its launch.  B = 0 launches nothing; frames[b] = 0 writes the zeros
 * alone.  No atomics: two launches give equal bits, an utterance alone or in a batch gives equal bits.  Defaults of the package,
 * plausible but this project's own: r_g = 0.75, r_l = -0.85, mu = 0.999, min_area = 1e-4.
 * Left out: a nasal branch, wall vibration and frequency-dependent losses, a two-mass glottis, more than 64 sections. */
int as_vt_glottal_source(const double* f0, const double* voiced_amp, const double* asp_amp, const int32_t* frames, int32_t B,
                         int32_t T, int32_t S, double sample_rate, uint64_t seed, double rise, double fall, double* source,
                         int64_t pitch, int32_t* status, void* stream);
int as_vt_waveguide(const double* areas, int64_t a_utt, int64_t a_frame, int64_t a_sec, const int32_t* sections,
                    const int32_t* frames, int32_t B, int32_t T, int32_t Kmax, int32_t S, const double* source,
                    const int32_t* inject_section, const double* inject_gain, uint64_t seed, double r_g, double r_l, double mu,
                    double min_area, int32_t radiation, double* out64, float* out32, int64_t pitch, int32_t* status, void* stream);

/* Exact t-SNE of the recogniser's features (artspeech_amd/csrc/tsne.hip).  The reference draws model_features.pdf with
 * sklearn.manifold.TSNE(n_components=2).fit_transform (phoneme_recognition/__init__.py:355-356); the four entry points below are
 * that routine's device work, stage by stage.  No float atomics; every sum that crosses a workgroup goes through the workspace
 * and is added in an order that depends on N alone: equal inputs give equal bits.  One workspace of as_tsne_workspace_bytes(N)
 * bytes (16-byte aligned; too small: AS_ERR_WORKSPACE) serves as_tsne_joint_p and as_tsne_iterate; it need not be cleared and
 * nothing in it has to survive between calls.  2 <= N <= 16384 (two (N, N) float32 matrices of 1 GiB each at the limit); a
 * larger N is refused with AS_ERR_BAD_ARG before anything is launched -- there is no second path.  Only the rows of one slab
 * of Y (at most 2048 points, 16 KiB) are ever staged in LDS, so the limit is the matrices', not the LDS's.
 *
 * as_tsne_sqdist (:355-356; sklearn.metrics.pairwise_distances(X, metric="euclidean", squared=True) of TSNE._fit):
 *     dist[i][j] = sum_k (x[i ldx + k] - x[j ldx + k])^2 by direct differences, one float32 chain over k = 0 .. D-1 (not the
 *     Gram form, which cancels for near-duplicate frames).  dist is (N, N) contiguous, exactly symmetric, its diagonal exactly 0.
 * as_tsne_joint_p (:355-356; sklearn.manifold._t_sne._joint_probabilities and _utils._binary_search_perplexity):
 *     per row the bisection on the precision beta in float64 (beta = 1 first, at most 100 steps, |H - log perplexity| <= 1e-5,
 *     scikit-learn's doubling / halving while an end of the interval is open), then
 *     P = max((C + C') / max(sum(C + C'), eps), eps), eps = 2^-52, stored as (N, N) float32, exactly symmetric, diagonal 0.
 *     dist must be symmetric (as as_tsne_sqdist writes it).  beta [N], entropy [N] (H in nats at the last step: the value of the
 *     stopping rule) are float64, steps [N] int32 (evaluations of H, 1 .. 100).  0 < perplexity < N.
 * as_tsne_iterate (:355-356; sklearn.manifold._t_sne._kl_divergence and _gradient_descent):
 *     n_iters iterations of  grad_i = 4 (exaggeration sum_j p_ij num_ij (y_i - y_j) - sum_j num_ij^2 (y_i - y_j) / Z),
 *     num_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} num_ij;  gains += 0.2 where update grad < 0, else gains *= 0.8, clipped at
 *     min_gain;  update = momentum update - learning_rate gains grad;  Y += update -- two launches per iteration on `stream`, no host
 *     synchronisation.  P (as as_tsne_joint_p writes it: symmetric) is read once per iteration and never rescaled.  Y, update and
 *     gains are (N, 2) float32 and updated in place.  log is (n_iters, 3) float64: |grad|_2, |gains grad|_2 (the norm
 *     scikit-learn's min_grad_norm test sees: it scales grad in place first) and the KL divergence
 *     2 sum_{i<j} p_ij log(max(p_ij, eps) / max(num_ij / Z, eps)) of the UNexaggerated P at the Y the iteration started from, or
 *     NaN: the KL is a pass of its own (two more launches) on iteration k of the call where (it0 + k + 1) % kl_every == 0
 *     (kl_every > 0) or, with kl_last, k == n_iters - 1.  grad (N, 2), optional: the last iteration's gradient. */
int64_t as_tsne_workspace_bytes(int32_t N);
int as_tsne_sqdist(const float* x, int64_t ldx, int32_t N, int32_t D, float* dist, void* stream);
int as_tsne_joint_p(const float* dist, int32_t N, double perplexity, float* P, double* beta, double* entropy, int32_t* steps,
                    void* ws, int64_t ws_bytes, void* stream);
int as_tsne_iterate(const float* P, float* Y, float* update, float* gains, int32_t N, int32_t n_iters, int32_t it0,
                    int32_t kl_every, int32_t kl_last, float exaggeration, float momentum, float learning_rate, float min_gain,
                    float* grad, double* log, void* ws, int64_t ws_bytes, void* stream);

/* Optional per-kernel-phase timing with HIP events recorded on the launch stream (for bench.py's
 * roofline object).  as_profile_report writes "name count total_ms\n" lines (NUL terminated, truncated
 * to buflen) and returns the untruncated length; it waits for the recorded events to complete. */
void as_profile_enable(int32_t on);
void as_profile_reset(void);
/* Diagnostic: in-kernel cycle stamps of the fused head-layer kernels (lin_f32.hip).  buf = device array of
 * 8 x (number of workgroups of the next launches) uint64, or NULL to switch the stamps off (the default; a kernel
 * launched without a buffer executes no stamp).  Per workgroup: s_memtime at start, after the prologue's first wait,
 * after the main loop, at the end; s_memrealtime at start; HW_ID and XCC_ID registers.  Never used by the product path. */
void as_lin_debug_stamps(uint64_t* buf, int64_t max_workgroups);
/* Diagnostic: per-workgroup stamps of the GRU backward recurrences: buf = device array of 2 x (4 x 2 x B) uint64, or NULL
 * (default: no stamps).  Consecutive backward launches alternate between the two halves (a training step launches layer 1,
 * then layer 0: half 0 and half 1 after a call that reset the counter); per (direction, utterance):
 * {shader cycles, 100 MHz wall ticks, sequence length, wall start}. */
void as_gru_debug_stamps(uint64_t* buf);
int32_t as_profile_report(char* buf, int32_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* ARTSPEECH_HIP_H */
