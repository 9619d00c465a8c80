"""ctypes binding of libartspeech_hip.so (the C ABI declared in include/artspeech_hip.h).

There is NO CPU fallback: if the library is missing every op raises.  torch is imported first so that
the HIP runtime already loaded by torch (its bundled libamdhip64) is the one the library binds to.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must be loaded before the library: single HIP runtime per process)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libartspeech_hip.so")

c_f32p = C.c_void_p  # device pointers travel as integers (tensor.data_ptr())


class Dims(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("n_art", C.c_int32), ("embed", C.c_int32), ("hidden", C.c_int32),
                ("n_samp", C.c_int32), ("simple", C.c_int32)]


class Layout(C.Structure):
    _fields_ = [("embedding", C.c_int64),
                ("w_ih", C.c_int64 * 2), ("b_ih", C.c_int64 * 2), ("w_hh", C.c_int64 * 2), ("b_hh", C.c_int64 * 2),
                ("lin_w", C.c_int64), ("lin_b", C.c_int64),
                ("ln1_g", C.c_int64), ("ln1_b", C.c_int64), ("w1", C.c_int64), ("b1", C.c_int64),
                ("ln2_g", C.c_int64), ("ln2_b", C.c_int64), ("w2", C.c_int64), ("b2", C.c_int64),
                ("ln3_g", C.c_int64), ("ln3_b", C.c_int64), ("w3", C.c_int64), ("b3", C.c_int64),
                ("total", C.c_int64)]


class Opts(C.Structure):
    _fields_ = [("gru_dropout", C.c_float), ("dropout_seed", C.c_uint64), ("dout_presigmoid", C.c_int32),
                ("defer_dw2", C.c_int32), ("fold_wait_event", C.c_void_p),
                ("loss_targets", C.c_void_p), ("loss_tgt_T", C.c_int64), ("loss_scale", C.c_float), ("loss_out", C.c_void_p),
                ("loss_dout", C.c_void_p)]


class Gemm(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("bias", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("a_i", C.c_int64), ("a_k", C.c_int64), ("b_j", C.c_int64), ("b_k", C.c_int64), ("ldc", C.c_int64),
                ("batch", C.c_int32), ("a_batch", C.c_int64), ("b_batch", C.c_int64), ("c_batch", C.c_int64),
                ("bias_batch", C.c_int64), ("act", C.c_int32), ("accumulate", C.c_int32),
                ("b_kshift", C.c_int32), ("b_kT", C.c_int32),
                ("splitk_ws", C.c_void_p), ("splitk_ws_floats", C.c_int64), ("colsum", C.c_void_p),
                ("colsum_batch", C.c_int64), ("a_off", C.c_void_p), ("b_off", C.c_void_p), ("c_off", C.c_void_p),
                ("bias_off", C.c_void_p), ("precision", C.c_int32), ("b_kshift_batch", C.c_int32), ("cu_budget", C.c_int32),
                ("res", C.c_void_p), ("res_ld", C.c_int64), ("res_batch", C.c_int64), ("res_off", C.c_void_p),
                ("mask_bits", C.c_void_p), ("mask_batch", C.c_int64), ("relu_bits", C.c_void_p), ("relu_bits_batch", C.c_int64),
                ("k_seg", C.c_int32), ("a_seg_off", C.c_void_p), ("b_seg_off", C.c_void_p), ("k_tri", C.c_int32)]


class MultiMlp(C.Structure):
    _fields_ = [("groups", C.c_int32), ("rows", C.c_int32), ("layers", C.c_int32), ("h1", C.c_int32), ("h2", C.c_int32),
                ("k_max", C.c_int32), ("n_max", C.c_int32), ("latent", C.c_int32),
                ("dims", C.c_void_p), ("params", C.c_void_p), ("in_mode", C.c_int32), ("in_scale", C.c_float),
                ("x", C.c_void_p), ("x_r", C.c_int64), ("x_g", C.c_int64), ("in_idx", C.c_void_p),
                ("out_mode", C.c_int32), ("act", C.c_int32), ("y", C.c_void_p), ("y_r", C.c_int64), ("y_g", C.c_int64),
                ("out_idx", C.c_void_p), ("own_ptr", C.c_void_p), ("own", C.c_void_p), ("win", C.c_void_p),
                ("ws", C.c_void_p), ("ws_floats", C.c_int64), ("dy", C.c_void_p), ("dx", C.c_void_p), ("dparams", C.c_void_p)]


class Pca(C.Structure):
    _fields_ = [("groups", C.c_int32), ("features", C.c_int32), ("k_max", C.c_int32), ("batch", C.c_int32),
                ("k", C.c_void_p), ("x", C.c_void_p), ("rows", C.c_int64), ("x_r", C.c_int64), ("x_g", C.c_int64),
                ("order", C.c_void_p), ("n_seen", C.c_int64), ("state", C.c_void_p),
                ("components", C.c_void_p), ("singular_values", C.c_void_p), ("explained_variance", C.c_void_p),
                ("explained_variance_ratio", C.c_void_p), ("noise_variance", C.c_void_p),
                ("ws", C.c_void_p), ("ws_floats", C.c_int64)]


class Stream(C.c_void_p):
    """Argtype of the trailing `void* stream` of a launching entry point: a void pointer like any other to ctypes, and the
    mark by which call() knows to append the stream."""
    from_param = C.c_void_p.from_param   # (a subclass's own from_param would turn away plain c_void_p instances: stream_ptr())


_P, _S, _I32, _I64, _F, _D = C.c_void_p, Stream, C.c_int32, C.c_int64, C.c_float, C.c_double
_DIMS, _LAY = C.POINTER(Dims), C.POINTER(Layout)

# name -> (restype, argtypes); every symbol include/artspeech_hip.h declares
PROTOTYPES = {
    "as_version": (C.c_char_p, []),
    "as_arch": (C.c_char_p, []),
    "as_last_error": (C.c_char_p, []),
    "as_artspeech_layout": (_I32, [_DIMS, _LAY]),
    "as_artspeech_workspace_floats": (_I64, [_DIMS, _I32, _I32]),
    "as_artspeech_fwd": (_I32, [_DIMS, _P, _P, _I64, _P, _I32, _I32, _P, _P, _I32, C.POINTER(Opts), _S]),
    "as_artspeech_bwd": (_I32, [_DIMS, _P, _P, _I64, _P, _I32, _I32, _P, _P, _P, _P, C.POINTER(Opts), _S]),
    "as_artspeech_dw2": (_I32, [_DIMS, _P, _I32, _I32, _P, _P, _S]),
    "as_gru_bidir_fwd": (_I32, [_P, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _P, _P, _S]),
    "as_gru_bidir_bwd": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _S]),
    "as_gemm_f32": (_I32, [C.POINTER(Gemm), _S]),
    "as_linear_planes_floats": (_I64, [_I32, _I32]),
    "as_linear_fwd": (_I32, [_P, _I64, _P, _I64, _P, _P, _I64, _I32, _I32, _I32, _I32, _P, _S]),
    "as_layernorm_fwd_blockres": (_I32, [_P, _P, _P, _P, _I32, _I64, _I32, _I32, _S]),
    "as_head_workspace_floats": (_I64, [_DIMS, _I64]),
    "as_head_fwd": (_I32, [_DIMS, _LAY, _P, _P, _I64, _P, _P, _I32, _S]),
    "as_head_bwd": (_I32, [_DIMS, _LAY, _P, _P, _P, _I64, _P, _P, _P, _S]),
    "as_euclid_fwd": (_I32, [_P, _P, _I64, _I32, _I32, _P, _S]),
    "as_euclid_bwd": (_I32, [_P, _P, _P, _I64, _I32, _I32, _P, _S]),
    "as_euclid_masked_partials": (_I32, []),
    "as_euclid_masked_fwd_bwd": (_I32, [_P, _P, _I64, _P, _I32, _I32, _I32, _I32, _F, _P, _P, _P, _S]),
    "as_euclid_masked_fwd_bwd_presigmoid": (_I32, [_P, _P, _I64, _P, _I32, _I32, _I32, _I32, _F, _P, _P, _P, _S]),
    "as_p2cp_fwd": (_I32, [_P, _I64, _I64, _I64, _I32, _P, _I64, _I64, _I64, _I32, _I64, _P, _S]),
    "as_p2cp_bwd": (_I32, [_P, _I64, _I64, _I64, _I32, _P, _I64, _I64, _I64, _I32, _I64, _P, _P, _I64, _I64, _I64, _P, _I64, _I64, _I64,
                           _S]),
    "as_p2cp_masked_partials": (_I32, []),
    "as_p2cp_masked_fwd_bwd": (_I32, [_P, _P, _I64, _P, _I32, _I32, _I32, _I32, _F, _P, _P, _P, _S]),
    "as_p2cp_utterance_mean": (_I32, [_P, _P, _I32, _I32, _I32, _F, _P, _S]),
    "as_pearson_fwd": (_I32, [_P, _I64, _I64, _P, _I64, _I64, _I32, _I32, _I32, _I32, _F, _P, _P, _S]),
    "as_tract_variables_fwd": (_I32, [_P, _I64, _I32, _I32, _P, _I32, _P, _P, _P, _P, _S]),
    "as_area_function_fwd": (_I32, [_P, _P, _I64, _I64, _I64, _I64, _I32, _D, _D, _P, _P, _S]),
    "as_evenly_spaced_fx": (_I32, [_P, _P, _I64, _I32, _I32, _P, _S]),
    "as_adam_step": (_I32, [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _I64, _F, _S]),
    "as_dropout_fwd": (_I32, [_P, _P, _I64, _F, C.c_uint64, _S]),
    "as_layernorm_fwd": (_I32, [_P, _P, _P, _P, _P, _P, _P, _I64, _I32, _I64, _S]),
    "as_fold_ln": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _S]),
    "as_attn_softmax": (_I32, [_P, _I64, _I32, _I32, _I32, _I32, _F, _P, _P, _S]),
    "as_embed_posenc": (_I32, [_P, _I64, _P, _P, _P, _I64, _I32, _I32, _S]),
    "as_attn_softmax_bwd": (_I32, [_P, _P, _I64, _I32, _I32, _F, _S]),
    "as_attention_supported": (_I32, [_I32, _I32, _I32, _I32]),
    "as_attention_fwd": (_I32, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _S]),
    "as_attention_fwd_causal": (_I32, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _S]),
    "as_attention_bwd_ds": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _S]),
    "as_attention_bwd_ds_causal": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _F, _S]),
    "as_group_reduce": (_I32, [_P, _P, _I32, _I32, _I64, _P, _S]),
    "as_layernorm_bwd": (_I32, [_P, _P, _P, _P, _P, _I64, _I32, _S]),
    "as_unfold_ln": (_I32, [_P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _S]),
    "as_relu_bwd": (_I32, [_P, _P, _P, _I64, _S]),
    "as_add": (_I32, [_P, _P, _P, _I64, _S]),
    "as_row_scale": (_I32, [_P, _P, _P, _I64, _I32, _S]),
    "as_copy_f32": (_I32, [_P, _P, _I64, _S]),
    "as_set_overlap": (None, [_I32]),
    "as_set_matrix_arith": (None, [_I32]),
    "as_get_matrix_arith": (_I32, []),
    "as_set_head_short_k": (None, [_I32]),
    "as_set_lin_out_row_epilogue": (None, [_I32]),
    "as_conv3x3_stem": (_I32, [_P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _S]),
    "as_conv3x3_c32": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _S]),
    "as_ln_feat_gelu": (_I32, [_P, _P, _P, _P, _I64, _I32, _I32, _S]),
    "as_gelu": (_I32, [_P, _P, _I64, _S]),
    "as_lstm_bidir_fwd": (_I32, [_P, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _P, _P, _S]),
    "as_lstm_bidir_bwd": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _S]),
    "as_gru_unidir_fwd": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _S]),
    "as_gru_unidir_fwd_gates": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _S]),
    "as_gru_unidir_bwd": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P, _S]),
    "as_ln_feat_gelu_bwd": (_I32, [_P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _S]),
    "as_conv3x3_stem_bwd": (_I32, [_P, _P, _P, _I64, _I64, _I64, _I64, _I32, _I32, _I32, _I32, _S]),
    "as_gelu_bwd": (_I32, [_P, _P, _P, _P, _I64, _I32, _S]),
    "as_conv3x3_c32_wgrad": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _I64, _S]),
    "as_conv3x3_stem_wgrad": (_I32, [_P, _I64, _I64, _I64, _I64, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _I64, _S]),
    "as_ln_feat_gelu_param_grad": (_I32, [_P, _P, _P, _P, _I64, _I32, _I32, _P, _P, _P, _I64, _S]),
    "as_layernorm_param_grad": (_I32, [_P, _P, _I64, _I32, _P, _P, _P, _I64, _S]),
    "as_ctc_workspace_floats": (_I64, [_I32, _I32, _I32]),
    "as_ctc_loss": (_I32, [_P, _I64, _I64, _I32, _I32, _I32, _I32, _P, _I64, _P, _P, _I32, _I32, _I32, _P, _I64, _P, _S]),
    "as_ctc_grad": (_I32, [_P, _I64, _I64, _I32, _I32, _I32, _I32, _P, _I64, _P, _P, _I32, _I32, _P, _I64, _P, _P, _I32, _P, _I64,
                           _I64, _S]),
    "as_ctc_align_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "as_ctc_align": (_I32, [_P, _I64, _I64, _I32, _I32, _I32, _I32, _P, _I64, _P, _P, _I32, _I32, _P, _I64, _P, _P, _P, _P, _P, _P, _S]),
    "as_ctc_beam_workspace_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "as_ctc_beam_search": (_I32, [_P, _I64, _I64, _I32, _I32, _I32, _I32, _P, _I32, _I32, _F, _I32, _I32, _F, _I32, _I32, _P, _P, _P, _P,
                                  _P, _I64, _S]),
    "as_decode_top1": (_I32, [_P, _I64, _I64, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _S]),
    "as_edit_distance": (_I32, [_P, _I32, _P, _P, _I32, _P, _I32, _P, _I32, _P, _S]),
    "as_align_workspace_bytes": (_I64, [_I32, _I32, _I32]),
    "as_align_counts": (_I32, [_P, _I32, _P, _P, _I32, _P, _I32, _P, _I32, _I32, _P, _P, _P, _I64, _S]),
    "as_confusion_counts": (_I32, [_P, _I32, _P, _I32, _P, _I32, _P, _I32, _I32, _P, _S]),
    "as_frame_ce_workspace_bytes": (_I64, [_I32, _I32]),
    "as_frame_ce_loss": (_I32, [_P, _I64, _I64, _I32, _I32, _I32, _P, _I64, _P, _P, _I64, _F, _P, _P, _P, _I64, _S]),
    "as_frame_ce_grad": (_I32, [_P, _I64, _I64, _I32, _I32, _I32, _P, _I64, _P, _P, _I64, _F, _P, _P, _P, _I32, _P, _I64, _I64, _S]),
    "as_frame_auroc": (_I32, [_P, _I64, _I64, _I32, _I32, _I32, _P, _I64, _P, _I64, _I32, _P, _P, _P, _S]),
    "as_intersect_semipolar_grid":(_I32, [_P, _P, _I64, _I32, _I32, _I32, _P, _P, _P, _S]),
    "as_artspeech_wait_head_grads": (_I32, [_P, _P]),
    "as_gather_pad_rows": (_I32, [_P, _P, _P, _I32, _I32, _I64, _I32, _D, _P, _S]),
    "as_lin_debug_stamps": (None, [_P, _I64]),
    "as_gru_debug_stamps": (None, [_P]),
    "as_multi_mlp_supported": (_I32, [_I32, _I32, _I32, _I32, _I32]),
    "as_multi_mlp_param_floats": (_I64, [_I32, _I32, _I32, _I32, _I32]),
    "as_multi_mlp_workspace_floats": (_I64, [C.POINTER(MultiMlp), _I32]),
    "as_multi_mlp_fwd": (_I32, [C.POINTER(MultiMlp), _S]),
    "as_multi_mlp_bwd": (_I32, [C.POINTER(MultiMlp), _S]),
    "as_pca_supported": (_I32, [_I32, _I32]),
    "as_pca_workspace_floats": (_I64, [C.POINTER(Pca)]),
    "as_pca_fit": (_I32, [C.POINTER(Pca), _S]),
    "as_token_runs_workspace_ints": (_I64, [_I64]),
    "as_token_runs": (_I32, [_P, _P, _P, _I32, _I64, _P, _P, _P, _P, _S]),
    "as_mean_contour_fit": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _S]),
    "as_mean_contour_fwd": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _S]),
    "as_mean_contour_weighted_fwd": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _S]),
    "as_pc_shapes_eval": (_I32, [_P, _P, _P, _P, _P, _I32, _P, _I32, _I64, _I32, _I32, _F, _P, _P, _P, _S]),
    "as_pc_eval_accumulate": (_I32, [_P, _I32, _P, _P, _I32, _P, _I64, _P, _I32, _S]),
    "as_segment_corr": (_I32, [_P, _P, _I64, _I32, _D, _P, _I32, _P, _P, _S]),
    "as_masked_mse_partials": (_I32, []),
    "as_masked_mse_fwd_bwd": (_I32, [_P, _P, _I64, _I64, _P, _I32, _P, _F, _P, _P, _P, _S]),
    "as_prepare_contours": (_I32, [_P, _P, _P, _I64, _I32, _I32, _F, _F, _F, _F, _P, _P, _I32, _P, _P, _P, _S]),
    "as_column_mean_std": (_I32, [_P, _I64, _I32, _P, _P, _P, _I64, _S]),
    "as_melspec_fwd": (_I32, [_P, _I64, _P, _I32, _I32, _I32, _P, _P, _I32, _F, _I32, _F, _P, _I64, _P, _S]),
    "as_resample_span": (_I64, [_I64, _I32, _I32, _I32, _I32]),
    "as_resample_tile": (_I32, [_I32, _I32, _I32, _I32]),
    "as_resample_fwd": (_I32, [_P, _I32, _I64, _P, _I32, _I32, _I32, _P, _P, _I32, _I32, _I32, _I32, _F, _P, _I64, _I64, _P, _S]),
    "as_contour_spline": (_I32, [_P, _I64, _I64, _I64, _I64, _I32, _I32, _I32, _D, _I32, _P, _I32, _I32, _P, _I64, _P, _S]),
    "as_vocal_tract_tube": (_I32, [_P, _I64, _I64, _I64, _I64, _I64, _I32, _I32, _P, _I32, _I32, _P, _I32, _I32, _P, _I64, _P, _P, _P, _S]),
    "as_vt_acoustics": (_I32, [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I32, _D, _D, _I32, _I32, _D, _D, _D, _I32, _I32, _P, _P, _P, _P,
                              _P, _P, _S]),
    "as_vt_glottal_source": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _D, C.c_uint64, _D, _D, _P, _I64, _P, _S]),
    "as_vt_waveguide": (_I32, [_P, _I64, _I64, _I64, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, C.c_uint64, _D, _D, _D, _D, _I32, _P, _P,
                              _I64, _P, _S]),
    "as_tsne_workspace_bytes": (_I64, [_I32]),
    "as_tsne_sqdist": (_I32, [_P, _I64, _I32, _I32, _P, _S]),
    "as_tsne_joint_p": (_I32, [_P, _I32, _D, _P, _P, _P, _P, _P, _I64, _S]),
    "as_tsne_iterate": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F, _F, _F, _F, _P, _P, _P, _I64, _S]),
    "as_profile_enable": (None, [_I32]),
    "as_profile_reset": (None, []),
    "as_profile_report": (_I32, [C.c_char_p, _I32]),
}

COLUMN_STATS_PART_ROWS = 512   # AS_COLUMN_STATS_PART_ROWS of the header: sizes as_column_mean_std's workspace

# Every launching entry point (one that takes a stream) returns a status code, and so do these two.  The other int32 results
# are sizes, counts and yes/no answers (as_attention_supported among them, an `int` in the header) and are handed back.
STATUS_WITHOUT_STREAM = ("as_artspeech_layout", "as_artspeech_wait_head_grads")

_lib = None
_bound = {}   # name -> (function, takes a stream, returns a status code)
_slabs = {}


def lib():
    """The loaded library; raises (loudly) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m artspeech_amd.build` "
                "(hipcc --offload-arch=gfx950). artspeech_amd has no CPU fallback.")
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
            takes_stream = bool(args) and args[-1] is Stream
            _bound[name] = (fn, takes_stream, takes_stream or name in STATUS_WITHOUT_STREAM)
        _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().as_last_error().decode()
        raise RuntimeError(f"{what or 'artspeech_hip'} failed (code {rc}): {msg}")


def require_gpu(t, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"artspeech_amd: {name} must live on an MI355X device (got {t.device}); there is no CPU path")
    return t


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def call(name, *args, stream=None):
    """The one way into the library: PROTOTYPES[name](*args [, stream]).  A tensor goes as its device address (one that is not on
    a GPU raises before anything is launched), None as NULL, a ctypes Structure by reference; numbers, bytes and raw addresses
    pass as they are.  An entry point that launches gets the stream appended: the current stream of the current device, or
    `stream` (a torch.cuda.Stream or a raw handle).  A status code other than 0 raises with the library's message; sizes, counts
    and answers are returned.  Nothing here synchronises, allocates or copies."""
    if _lib is None:
        lib()
    fn, takes_stream, status = _bound[name]
    conv = []
    for a in args:
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                require_gpu(a, f"{name}: argument {len(conv)}")
            a = a.data_ptr()
        elif isinstance(a, C.Structure):
            a = C.byref(a)
        conv.append(a)
    if takes_stream:
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        elif isinstance(stream, torch.cuda.Stream):
            stream = stream.cuda_stream
        conv.append(stream)
    elif stream is not None:
        raise TypeError(f"{name} takes no stream")
    res = fn(*conv)
    if status and res != 0:
        check(res, name)
    return res


def layout(dims):
    lay = Layout()
    call("as_artspeech_layout", dims, lay)
    return lay


def gemm_desc(**fields):
    """A filled as_gemm descriptor: tensors become their device addresses, batch is 1 unless given."""
    g = Gemm()
    g.batch = 1
    for k, v in fields.items():
        if isinstance(v, torch.Tensor):
            if not v.is_cuda:
                require_gpu(v, f"as_gemm.{k}")
            v = v.data_ptr()
        setattr(g, k, v)
    return g


def gemm(**fields):
    call("as_gemm_f32", gemm_desc(**fields))


def slab(device, floats):
    """The device's workspace of `floats` floats for split-K slabs, stream-K pieces and partial sums (one per size: the kernels
    derive their split factors from the size they are given)."""
    key = (device, floats)
    if key not in _slabs:
        _slabs[key] = torch.empty(floats, dtype=torch.float32, device=device)
    return _slabs[key]


def contiguous(t):
    return t if t.is_contiguous() else t.contiguous()
