"""ctypes binding of libcogview_hip.so (see include/cogview_hip.h).

There is NO CPU fallback: if the shared library cannot be loaded every compute entry point raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# COGVIEW_HIP_LIB points the loader at another build of the same ABI (kernel experiments); default: in-tree
LIB_PATH = os.environ.get("COGVIEW_HIP_LIB") or os.path.join(_HERE, "lib", "libcogview_hip.so")

F16, BF16, F32 = 0, 1, 2
EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_DROPOUT, EPI_ABSMAX, EPI_ACCUM, EPI_COLSUM = 1, 2, 4, 8, 16, 32, 64
EPI_GELU_DAUX, EPI_MULAUX = 128, 256

_ERR = {1: "bad argument (shape / alignment / dtype)", 2: "kernel launch failure", 3: "unsupported combination"}


class CogviewHipError(RuntimeError):
    pass


class GemmDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("trans_a", C.c_int), ("trans_b", C.c_int),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("A", C.c_void_p), ("lda", C.c_int),
        ("B", C.c_void_p), ("ldb", C.c_int),
        ("C", C.c_void_p), ("ldc", C.c_int),
        ("out_f32", C.c_int), ("flags", C.c_int),
        ("bias", C.c_void_p),
        ("aux", C.c_void_p), ("ldaux", C.c_int),
        ("absmax", C.c_void_p),
        ("dropout_p", C.c_float), ("seed", C.c_uint64), ("stream_id", C.c_uint64),
        ("splitk", C.c_int), ("kernel_variant", C.c_int),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("colsum_partial", C.c_void_p),
        ("dropout_row0", C.c_longlong),
    ]


class AttnDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("B", C.c_int), ("H", C.c_int), ("s_q", C.c_int), ("s_k", C.c_int),
        ("head_dim", C.c_int), ("sep", C.c_int),
        ("scale", C.c_float), ("dropout_p", C.c_float), ("seed", C.c_uint64), ("stream_id", C.c_uint64),
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
        ("dout", C.c_void_p), ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p),
        ("lse", C.c_void_p), ("dvec", C.c_void_p),
        ("q_bs", C.c_longlong), ("k_bs", C.c_longlong), ("v_bs", C.c_longlong), ("o_bs", C.c_longlong),
        ("do_bs", C.c_longlong), ("dq_bs", C.c_longlong), ("dk_bs", C.c_longlong), ("dv_bs", C.c_longlong),
        ("q_rs", C.c_int), ("k_rs", C.c_int), ("v_rs", C.c_int), ("o_rs", C.c_int),
        ("do_rs", C.c_int), ("dq_rs", C.c_int), ("dk_rs", C.c_int), ("dv_rs", C.c_int),
        ("colsum_partial", C.c_void_p),
        ("kv_index", C.c_void_p), ("kv_index_bs", C.c_longlong),
        ("kv_index_gs", C.c_longlong), ("sparse_window", C.c_int), ("sparse_pivots", C.c_int), ("sparse_pivot_bias", C.c_float),
        ("keep_bits", C.c_void_p),
        ("mask", C.c_void_p), ("mask_bs", C.c_longlong),
    ]


class LnPrologue(C.Structure):
    _fields_ = [
        ("z", C.c_void_p), ("z_absmax", C.c_void_p),
        ("gamma_post", C.c_void_p), ("beta_post", C.c_void_p), ("residual", C.c_void_p), ("t_out", C.c_void_p),
        ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("eps", C.c_float), ("stream_f32", C.c_int),
    ]


class W8Weight(C.Structure):
    _fields_ = [("q", C.c_void_p), ("ldq", C.c_int), ("scale", C.c_void_p)]


class W4Weight(C.Structure):
    _fields_ = [("q", C.c_void_p), ("ldq", C.c_int), ("scale", C.c_void_p), ("lds", C.c_int)]


class AttnDecodeDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("B", C.c_int), ("H", C.c_int), ("capacity", C.c_int), ("head_dim", C.c_int),
        ("scale", C.c_float),
        ("qkv", C.c_void_p), ("qkv_bs", C.c_longlong),
        ("cache", C.c_void_p), ("cache_bs", C.c_longlong), ("cache_rs", C.c_int),
        ("out", C.c_void_p), ("out_bs", C.c_longlong),
        ("pos", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("skip_combine", C.c_int),
        ("first", C.c_void_p),
    ]


class AttnDecodeChunkDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("B", C.c_int), ("H", C.c_int), ("capacity", C.c_int), ("head_dim", C.c_int),
        ("m", C.c_int),
        ("scale", C.c_float),
        ("qkv", C.c_void_p), ("qkv_rs", C.c_longlong),
        ("cache", C.c_void_p), ("cache_bs", C.c_longlong), ("cache_rs", C.c_int),
        ("out", C.c_void_p), ("out_rs", C.c_longlong),
        ("pos", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("skip_combine", C.c_int),
        ("first", C.c_void_p),
    ]


class AttnDecodeKv8Desc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("B", C.c_int), ("H", C.c_int), ("capacity", C.c_int), ("head_dim", C.c_int),
        ("scale", C.c_float),
        ("qkv", C.c_void_p), ("qkv_bs", C.c_longlong),
        ("kv_q", C.c_void_p), ("kv_q_bs", C.c_longlong),
        ("kv_scale", C.c_void_p), ("kv_scale_bs", C.c_longlong),
        ("out", C.c_void_p), ("out_bs", C.c_longlong),
        ("pos", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("skip_combine", C.c_int),
        ("first", C.c_void_p),
    ]


class AttnDecodeChunkKv8Desc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("B", C.c_int), ("H", C.c_int), ("capacity", C.c_int), ("head_dim", C.c_int),
        ("m", C.c_int),
        ("scale", C.c_float),
        ("qkv", C.c_void_p), ("qkv_rs", C.c_longlong),
        ("kv_q", C.c_void_p), ("kv_q_bs", C.c_longlong),
        ("kv_scale", C.c_void_p), ("kv_scale_bs", C.c_longlong),
        ("out", C.c_void_p), ("out_rs", C.c_longlong),
        ("pos", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("skip_combine", C.c_int),
        ("first", C.c_void_p),
    ]


class AdamDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int),
        ("params", C.c_void_p), ("grads", C.c_void_p),
        ("master", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("chunk_start", C.c_void_p), ("chunk_len", C.c_void_p), ("chunk_group", C.c_void_p), ("nchunks", C.c_int),
        ("lr", C.c_float * 8), ("weight_decay", C.c_float * 8),
        ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("step", C.c_int), ("bias_correction", C.c_int), ("adam_w_mode", C.c_int),
        ("beta1_d", C.c_double), ("beta2_d", C.c_double),
        ("inv_loss_scale", C.c_float), ("max_grad_norm", C.c_float),
        ("stats", C.c_void_p), ("norm_sumsq_override", C.c_void_p),
    ]


class ConvDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int), ("B", C.c_int), ("IH", C.c_int), ("IW", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
        ("relu", C.c_int),
        ("in", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("rgb_w", C.c_void_p), ("rgb_partial", C.c_void_p),
        ("relu_in", C.c_int), ("residual", C.c_void_p), ("relu_residual", C.c_int),
        ("precision", C.c_int), ("w_limbs", C.c_void_p),
    ]


class ConvWgradDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int), ("B", C.c_int), ("IH", C.c_int), ("IW", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
        ("splits", C.c_int),
        ("x", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("relu_x", C.c_int), ("topologies", C.c_int),
    ]


class SampleDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("rows", C.c_int), ("vocab", C.c_int), ("row_stride", C.c_int64),
        ("logits", C.c_void_p),
        ("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float), ("allow_lo", C.c_int), ("allow_hi", C.c_int),
        ("seed", C.c_uint64), ("offset", C.c_void_p),
        ("ids", C.c_void_p), ("logp", C.c_void_p), ("scores", C.c_void_p), ("probs", C.c_void_p),
        ("tok", C.c_void_p), ("pos", C.c_void_p), ("pos_index", C.c_void_p), ("table", C.c_void_p), ("capacity", C.c_int),
        ("out_tokens", C.c_void_p), ("out_len", C.c_int64), ("out_base", C.c_int64),
        ("counter", C.c_void_p),
        ("given_stride", C.c_int64),
        ("given", C.c_void_p),
    ]


class ScoreDesc(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("rows", C.c_int), ("vocab", C.c_int), ("row_stride", C.c_int64),
        ("logits", C.c_void_p), ("target", C.c_void_p),
        ("allow_lo", C.c_int), ("allow_hi", C.c_int),
        ("group", C.c_int),
        ("logp", C.c_void_p),
        ("scores", C.c_void_p),
    ]


CONV_4X4_S2, CONV_1X1, CONVT_4X4_S2, CONV_3X3_S1 = 0, 1, 2, 3
CONV_FP32, CONV_BF16X3 = 0, 1          # cogv_conv_desc.precision

_vp, _i, _f, _u64, _i64, _sz = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_int64, C.c_size_t

# name -> (restype, argtypes).  Mirrors include/cogview_hip.h one-to-one (tests/test_abi.py checks this).
SIGNATURES = {
    "cogv_version": (_i, []),
    "cogv_arch": (C.c_char_p, []),
    "cogv_gemm": (_i, [C.POINTER(GemmDesc), _vp]),
    "cogv_gemm_workspace_bytes": (_sz, [C.POINTER(GemmDesc)]),
    "cogv_gemm_pick_splitk": (_i, [_i, _i, _i]),
    "cogv_gemm_grouped": (_i, [C.POINTER(GemmDesc), _i, _vp]),
    "cogv_gemm_colsum_rows": (_i, [_i]),
    "cogv_colsum_finalize": (_i, [_i, _vp, _i, _i, _vp, _i, _vp]),
    "cogv_gemm_pick_splitk_tiles": (_i, [_i, _i]),
    "cogv_sandwich_ln_fwd": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp]),
    "cogv_sandwich_ln_bwd": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _u64, _u64,
                                  _vp, _sz, _i, _vp]),
    "cogv_sandwich_ln_bwd_marked": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _sz, _i, _vp]),
    "cogv_ln_bwd_workspace_bytes": (_sz, [_i, _i]),
    "cogv_sandwich_ln_bwd_pair": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f,
                                       _vp, _sz, _vp]),
    "cogv_ln_bwd_pair_workspace_bytes": (_sz, [_i, _i]),
    "cogv_ln_bwd_num_blocks": (_i, [_i]),
    "cogv_ln_bwd_plan": (_i, [_i, _i, _i, _f, _i, _i, C.POINTER(C.c_int)]),
    "cogv_ln_bwd_pair_plan": (_i, [_i, _i, _f, C.POINTER(C.c_int)]),
    "cogv_gemm_reserve_cus": (_i, [_i]),
    "cogv_gemm_plan": (_i, [C.POINTER(GemmDesc), _i, _i, C.POINTER(C.c_int)]),
    "cogv_attention_fwd": (_i, [C.POINTER(AttnDesc), _vp]),
    "cogv_attention_bwd": (_i, [C.POINTER(AttnDesc), _vp]),
    "cogv_attention_plan": (_i, [C.POINTER(AttnDesc), _i, C.POINTER(C.c_int)]),
    "cogv_gemv_ln": (_i, [C.POINTER(GemmDesc), C.POINTER(LnPrologue), _vp]),
    "cogv_gemv_attn": (_i, [C.POINTER(GemmDesc), _vp, _i, _i, _vp]),
    "cogv_attention_decode": (_i, [C.POINTER(AttnDecodeDesc), _vp]),
    "cogv_attention_decode_chunk": (_i, [C.POINTER(AttnDecodeChunkDesc), _vp]),
    "cogv_quantize_rows_e4m3": (_i, [_i, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "cogv_gemm_w8": (_i, [C.POINTER(GemmDesc), C.POINTER(W8Weight), _vp]),
    "cogv_gemv_ln_w8": (_i, [C.POINTER(GemmDesc), C.POINTER(LnPrologue), C.POINTER(W8Weight), _vp]),
    "cogv_gemv_attn_w8": (_i, [C.POINTER(GemmDesc), C.POINTER(W8Weight), _vp, _i, _i, _vp]),
    "cogv_gemv_plan": (_i, [_i, C.POINTER(GemmDesc), C.POINTER(W8Weight), _i, C.POINTER(C.c_int)]),
    "cogv_quantize_rows_mxfp4": (_i, [_i, _vp, _i, _i, _i, _vp, _i, _vp, _i, _vp]),
    "cogv_gemm_w4": (_i, [C.POINTER(GemmDesc), C.POINTER(W4Weight), _vp]),
    "cogv_gemv_ln_w4": (_i, [C.POINTER(GemmDesc), C.POINTER(LnPrologue), C.POINTER(W4Weight), _vp]),
    "cogv_gemv_attn_w4": (_i, [C.POINTER(GemmDesc), C.POINTER(W4Weight), _vp, _i, _i, _vp]),
    "cogv_gemv_w4_plan": (_i, [_i, C.POINTER(GemmDesc), C.POINTER(W4Weight), _i, C.POINTER(C.c_int)]),
    "cogv_gemm_rows": (_i, [C.POINTER(GemmDesc), _vp]),
    "cogv_gemm_rows_plan": (_i, [C.POINTER(GemmDesc), C.POINTER(C.c_int)]),
    "cogv_gemm_rows_w8": (_i, [C.POINTER(GemmDesc), C.POINTER(W8Weight), _vp]),
    "cogv_gemm_rows_w4": (_i, [C.POINTER(GemmDesc), C.POINTER(W4Weight), _vp]),
    "cogv_gemm_rows_w8_plan": (_i, [C.POINTER(GemmDesc), C.POINTER(W8Weight), C.POINTER(C.c_int)]),
    "cogv_gemm_rows_w4_plan": (_i, [C.POINTER(GemmDesc), C.POINTER(W4Weight), C.POINTER(C.c_int)]),
    "cogv_kv_quantize_e4m3": (_i, [_i, _vp, _i64, _i64, _i, _i, _i, _vp, _i64, _vp, _i64, _i, _i, _vp]),
    "cogv_attention_decode_kv8": (_i, [C.POINTER(AttnDecodeKv8Desc), _vp]),
    "cogv_attention_decode_chunk_kv8": (_i, [C.POINTER(AttnDecodeChunkKv8Desc), _vp]),
    "cogv_attention_decode_workspace_bytes": (_sz, [_i, _i, _i]),
    "cogv_attention_keep_bits_bytes": (_sz, [_i, _i, _i, _i]),
    "cogv_sparse_slot_reduce": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i64, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "cogv_embedding_fwd": (_i, [_i, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i, _f, _u64, _u64, _i, _vp]),
    "cogv_embedding_bwd": (_i, [_i, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _i, _f, _u64, _u64, _vp, _sz, _i, _vp]),
    "cogv_embedding_bwd_workspace_bytes": (_sz, [_i64, _i64]),
    "cogv_gelu_fwd": (_i, [_i, _vp, _vp, _sz, _vp]),
    "cogv_gelu_bwd": (_i, [_i, _vp, _vp, _vp, _sz, _vp]),
    "cogv_dropout": (_i, [_i, _vp, _vp, _sz, _f, _u64, _u64, _vp, _vp]),
    "cogv_add": (_i, [_i, _vp, _vp, _vp, _sz, _vp, _vp]),
    "cogv_add_stream": (_i, [_i, _vp, _vp, _vp, _sz, _vp, _vp]),
    "cogv_scale": (_i, [_i, _vp, _vp, _sz, _f, _vp]),
    "cogv_absmax": (_i, [_i, _vp, _sz, _vp, _vp]),
    "cogv_colsum": (_i, [_i, _vp, _i, _i, _i, _vp, _i, _vp, _sz, _vp]),
    "cogv_colsum_workspace_bytes": (_sz, [_i, _i]),
    "cogv_ce_fwd": (_i, [_i, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "cogv_ce_bwd": (_i, [_i, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "cogv_grad_stats": (_i, [_i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "cogv_grad_stats_workspace_bytes": (_sz, []),
    "cogv_adamw_step": (_i, [C.POINTER(AdamDesc), _vp]),
    "cogv_cast_flat": (_i, [_i, _vp, _vp, _sz, _vp]),
    "cogv_cast_flat_back": (_i, [_i, _vp, _vp, _sz, _vp]),
    "cogv_conv2d_nhwc_f32": (_i, [C.POINTER(ConvDesc), _vp]),
    "cogv_conv_split_weights": (_i, [_vp, _vp, _sz, _vp]),
    "cogv_rgb_finalize_f32": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_float), _vp]),
    "cogv_vq_argmin_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "cogv_nchw3_to_nhwc4_f32": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "cogv_embed_code_f32": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp]),
    "cogv_sample_logits": (_i, [C.POINTER(SampleDesc), _vp]),
    "cogv_score_targets": (_i, [C.POINTER(ScoreDesc), _vp]),
    "cogv_conv1x1_to_rgb_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_float), _vp]),
    "cogv_conv_wgrad_plan": (_i, [C.POINTER(ConvWgradDesc), C.POINTER(C.c_int)]),
    "cogv_conv_wgrad_workspace_bytes": (_sz, [C.POINTER(ConvWgradDesc)]),
    "cogv_conv_wgrad_nhwc_f32": (_i, [C.POINTER(ConvWgradDesc), _vp]),
    "cogv_relu_bias_bwd_workspace_bytes": (_sz, [_i64, _i]),
    "cogv_relu_bias_bwd_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i64, _i, _vp]),
    "cogv_vq_code_stats_workspace_bytes": (_sz, [_i, _i, _i]),
    "cogv_vq_code_stats_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _vp]),
    "cogv_vq_ema_update_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _i, _i, _vp]),
    "cogv_vq_ste_bwd_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "cogv_resample_coeffs": (_i, [_i, _i, _vp, _vp, _vp, _i]),
    "cogv_image_prep_plan": (_i, [_i, _i, _i, C.POINTER(C.c_int)]),
    "cogv_image_prep_u8": (_i, [_vp, _sz, _vp, _vp, _vp, _sz, _i, _i, _vp, _vp, _vp]),
    "cogv_sr_patches_nhwc4_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "cogv_image_grid_plan": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int64)]),
    "cogv_image_range_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "cogv_image_grid_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, C.c_double, _i, _vp, C.c_double, C.c_double, _vp, _sz, _vp]),
}

_lib = None


def lib():
    """Return the loaded library, loading it on first use.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CogviewHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  cogview_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError here == ABI drift, fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        raise CogviewHipError(f"{what} failed: {_ERR.get(rc, rc)}")


OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
GEMV_PLAIN, GEMV_ATTN, GEMV_LN = 0, 1, 2
GEMV_PLAN_INTS = 11
GEMM_PLAN_INTS = 17
GEMM_PLAN_FIELDS = ("family", "generation", "tile_m", "tile_n", "tiles_m", "tiles_n", "splitk", "ktiles_per_split", "item_start", "items",
                    "grid_x", "grid_y", "threads", "lds", "reduce_blocks", "xp_ok", "layout")


def gemm_plan(descs, count=0, num_cus=0):
    """cogv_gemm_plan: (error code, one dict of GEMM_PLAN_FIELDS per problem) of what cogv_gemm (count 0: `descs` is one GemmDesc)
    or cogv_gemm_grouped (count >= 1: an array of them) would launch; host only, no pointer in a descriptor is read."""
    n = max(count, 1)
    out = (C.c_int * (GEMM_PLAN_INTS * n))()
    rc = lib().cogv_gemm_plan(descs if count else C.byref(descs), count, num_cus, out)
    return rc, [dict(zip(GEMM_PLAN_FIELDS, out[i * GEMM_PLAN_INTS:(i + 1) * GEMM_PLAN_INTS])) for i in range(n if rc == OK else 0)]


def _stand_in_desc(dtype, M, N, K, ldb=None):
    """the descriptor of a contiguous product for a plan query: the pointers are aligned stand-ins that nothing reads"""
    d = GemmDesc()
    d.dtype, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.splitk = dtype, M, N, K, K, K if ldb is None else ldb, N, 1
    d.A, d.B, d.C = 0x1000, 0x2000, 0x3000
    return d


def _stand_in_w8(K, ldq=None):
    w = W8Weight()
    w.q, w.ldq, w.scale = 0x2000, K if ldq is None else ldq, 0x4000
    return w


def _stand_in_w4(K, ldq=None, lds=None):
    w = W4Weight()
    w.q, w.ldq, w.scale, w.lds = 0x2000, K // 2 if ldq is None else ldq, 0x4000, K // 32 if lds is None else lds
    return w


def _plan_query(name, ints, *args):
    """(error code, the `ints` integers a plan query wrote: all -1 where it refused) of lib().<name>(*args, out)"""
    out = (C.c_int * ints)(*([-1] * ints))
    rc = getattr(lib(), name)(*args, out)
    return rc, list(out)


def gemv_plan(kind, dtype, M, N, K, w8=False, nsplit=1, ldb=None):
    """cogv_gemv_plan for a contiguous product of `kind` (GEMV_*): (error code, [generation, form, J | NWK, KCMAX | LMAX, guarded,
    MT, tiles per workgroup, two halves, threads, workgroups, dynamic LDS bytes]).  Host only: the pointers in the descriptors
    are aligned stand-ins that nothing reads.  w8: the product on an E4M3 weight; ldb: elements (bytes) between its rows."""
    d = _stand_in_desc(dtype, M, N, K, ldb)
    return _plan_query("cogv_gemv_plan", GEMV_PLAN_INTS, kind, C.byref(d), C.byref(_stand_in_w8(K, d.ldb)) if w8 else None, nsplit)


def gemv_w4_plan(kind, dtype, M, N, K, nsplit=1, ldq=None, lds=None):
    """cogv_gemv_w4_plan for a contiguous product of `kind` on an MXFP4 weight: (error code, the 11 integers of gemv_plan).  Host
    only.  ldq / lds: bytes between the rows of the codes (default K / 2) and of the block scales (default K / 32)."""
    return _plan_query("cogv_gemv_w4_plan", GEMV_PLAN_INTS, kind, C.byref(_stand_in_desc(dtype, M, N, K)), C.byref(_stand_in_w4(K, ldq, lds)), nsplit)


GEMM_ROWS_PLAN_INTS = 10
GEMM_ROWS_PLAN_FIELDS = ("row_groups", "waves_per_tile", "tiles", "weight_loads", "guarded", "x_staged", "threads", "grid", "lds", "pairs_in_flight")


def gemm_rows_plan(dtype, M, N, K, desc=None):
    """cogv_gemm_rows_plan for a contiguous product (or for the GemmDesc `desc` as it stands): (error code, the integers of
    GEMM_ROWS_PLAN_FIELDS; all -1 where the call is refused).  Host only: the pointers are aligned stand-ins that nothing reads."""
    d = _stand_in_desc(dtype, M, N, K) if desc is None else desc
    return _plan_query("cogv_gemm_rows_plan", GEMM_ROWS_PLAN_INTS, C.byref(d))


def gemm_rows_w8_plan(dtype, M, N, K, ldq=None, desc=None, w=None):
    """cogv_gemm_rows_w8_plan for a contiguous product on an E4M3 weight (or for the GemmDesc `desc` / W8Weight `w` as they
    stand): (error code, the integers of GEMM_ROWS_PLAN_FIELDS; all -1 where the call is refused).  Host only.  ldq: bytes
    between the rows of the codes (default K)."""
    d = _stand_in_desc(dtype, M, N, K) if desc is None else desc
    w = _stand_in_w8(d.K, ldq) if w is None else w
    return _plan_query("cogv_gemm_rows_w8_plan", GEMM_ROWS_PLAN_INTS, C.byref(d), C.byref(w))


def gemm_rows_w4_plan(dtype, M, N, K, ldq=None, lds=None, desc=None, w=None):
    """cogv_gemm_rows_w4_plan for a contiguous product on an MXFP4 weight (or for `desc` / the W4Weight `w` as they stand):
    (error code, the integers of GEMM_ROWS_PLAN_FIELDS; all -1 where the call is refused).  Host only.  ldq / lds: bytes between
    the rows of the codes (default K / 2) and of the block scales (default K / 32)."""
    d = _stand_in_desc(dtype, M, N, K) if desc is None else desc
    w = _stand_in_w4(d.K, ldq, lds) if w is None else w
    return _plan_query("cogv_gemm_rows_w4_plan", GEMM_ROWS_PLAN_INTS, C.byref(d), C.byref(w))


CONV_WGRAD_PLAN_INTS = 6
CONV_WGRAD_PLAN_FIELDS = ("splits", "span", "workgroups", "cout_tiles", "k_tiles", "parities")


def conv_wgrad_plan(kind, B, IH, IW, Cin, Cout, splits=0, relu_x=0, topologies=0):
    """cogv_conv_wgrad_plan: (error code, dict of CONV_WGRAD_PLAN_FIELDS; empty where the layer is refused) of what
    cogv_conv_wgrad_nhwc_f32 launches for that forward layer.  Host only.  topologies=1: CONV_3X3_S1 is planned too, and
    cout_tiles counts 32-wide tiles where Cout <= 32."""
    d = ConvWgradDesc()
    d.kind, d.B, d.IH, d.IW, d.Cin, d.Cout, d.splits = kind, B, IH, IW, Cin, Cout, splits
    d.relu_x, d.topologies = relu_x, topologies
    out = (C.c_int * CONV_WGRAD_PLAN_INTS)(*([-1] * CONV_WGRAD_PLAN_INTS))
    rc = lib().cogv_conv_wgrad_plan(C.byref(d), out)
    return rc, dict(zip(CONV_WGRAD_PLAN_FIELDS, out)) if rc == OK else {}


IMAGE_PREP_PLAN_INTS = 10
IMAGE_PREP_PLAN_FIELDS = ("nh", "nw", "top", "left", "taps_h", "taps_v", "band_rows", "seg_cols", "lds_rows", "lds_bytes")
IMAGE_PREP_MAX_TAPS = 65


def image_prep_plan(H, W, S):
    """cogv_image_prep_plan: (error code, dict of IMAGE_PREP_PLAN_FIELDS; empty where the image is refused) of what
    cogv_image_prep_u8 does with one H x W image at size S.  Host only."""
    out = (C.c_int * IMAGE_PREP_PLAN_INTS)(*([-1] * IMAGE_PREP_PLAN_INTS))
    rc = lib().cogv_image_prep_plan(H, W, S, out)
    return rc, dict(zip(IMAGE_PREP_PLAN_FIELDS, out)) if rc == OK else {}


def resample_coeffs(n_in, n_out, max_taps=IMAGE_PREP_MAX_TAPS):
    """cogv_resample_coeffs: (error code, xmin [n_out], count [n_out], k [n_out, max_taps]) as int32 numpy arrays (None where
    refused): Pillow's bilinear tables of one axis n_in -> n_out.  Host only."""
    import numpy as np
    if n_out <= 0 or max_taps <= 0:
        return ERR_ARG, None, None, None
    xmin, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    k = np.zeros((n_out, max_taps), np.int32)
    rc = lib().cogv_resample_coeffs(n_in, n_out, xmin.ctypes.data, count.ctypes.data, k.ctypes.data, max_taps)
    return (rc, xmin, count, k) if rc == OK else (rc, None, None, None)


IMAGE_GRID_PLAN_INTS = 6
IMAGE_GRID_PLAN_FIELDS = ("xmaps", "ymaps", "grid_h", "grid_w", "out_bytes", "range_bytes")
GRID_NORM_NONE, GRID_NORM_FIXED, GRID_NORM_RANGE, GRID_NORM_RANGE_EACH = 0, 1, 2, 3


def image_grid_plan(B, H, W, nrow=8, padding=2, scale_each=False, table=None):
    """cogv_image_grid_plan: (error code, dict of IMAGE_GRID_PLAN_FIELDS; empty where the call is refused) of the grid
    cogv_image_grid_u8 writes for B images of H x W.  table: the int32 [K, 8] source table as a numpy array, checked as the
    launches check it (None: geometry only).  Host only."""
    out = (C.c_int64 * IMAGE_GRID_PLAN_INTS)(*([-1] * IMAGE_GRID_PLAN_INTS))
    K = 0 if table is None else int(table.shape[0])
    rc = lib().cogv_image_grid_plan(None if table is None else table.ctypes.data, K, B, H, W, nrow, padding, int(bool(scale_each)), out)
    return rc, dict(zip(IMAGE_GRID_PLAN_FIELDS, out)) if rc == OK else {}
