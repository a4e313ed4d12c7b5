"""ctypes binding of ``libstreamformer_hip.so`` (the C ABI in ``include/streamformer_hip.h``).

There is no fallback: if the shared library is missing or does not load, importing this module
raises, and so does every product path that needs it.  ``torch`` is imported first on purpose — the
library is linked against ``libamdhip64.so.7`` by SONAME only, so it binds to the HIP runtime torch
has already loaded and shares its device context, allocator pointers and streams.
"""
from __future__ import annotations

import ctypes as C
import inspect
import os
import weakref

import torch  # noqa: F401  (must precede the CDLL below: shared HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libstreamformer_hip.so")
if os.environ.get("SF_LIB"):      # tools/ only: "lab" = the -DSF_LAB measurement build (`build.py --lab`), other names = A/B builds (`build.py --variant=name -D...`)
    LIB_PATH = os.path.join(_HERE, "libstreamformer_hip_%s.so" % os.environ["SF_LIB"])

SF_OK = 0
SF_ERR_INVALID, SF_ERR_STATE, SF_ERR_HIP, SF_ERR_WORKSPACE, SF_ERR_UNKNOWN_KEY, SF_ERR_CAPACITY = -1, -2, -3, -4, -5, -6
SF_F32, SF_BF16, SF_F16, SF_F64, SF_U8 = 0, 1, 2, 3, 4
SF_COMPUTE_BF16, SF_COMPUTE_BF16X3 = 0, 1


class SfConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "image_size", "patch_size", "num_channels", "num_frames", "hidden_size", "num_hidden_layers",
        "num_attention_heads", "intermediate_size", "hidden_act", "qkv_bias", "enable_causal_temporal",
        "add_lora_spatial")] + [("layer_norm_eps", C.c_float)]


class SfTextConfig(C.Structure):
    """sf_text_config: HF SiglipTextConfig as plain ints (act: 0 erf GELU, 1 tanh GELU, 2 ReLU)."""
    _fields_ = [(n, C.c_int32) for n in ("vocab", "positions", "hidden", "layers", "heads", "intermediate", "projection", "act")] + [
        ("eps", C.c_float)]


class SfConnectorConfig(C.Structure):
    """sf_connector_config: the LLaVA connector fields as plain ints (pool_mode 0 none, 1 average, 2 max, 3 bilinear; newline 0 no_token,
    1 one_token, 2 frame, 3 grid)."""
    _fields_ = [(n, C.c_int32) for n in ("in_dim", "out_dim", "depth", "pool_mode", "pool_stride", "newline")]


class SfOadConfig(C.Structure):
    """sf_oad_config: the LSTR stream detector's fields as plain ints (act 0 erf GELU, 2 ReLU; enc_queries -1 = encoder layers)."""
    _fields_ = [(n, C.c_int32) for n in ("d_in", "d_model", "heads", "ffn", "long_samples", "work_samples", "classes", "act",
                                         "linear_enabled", "enc_modules")] + [
        (n, C.c_int32 * 8) for n in ("enc_queries", "enc_layers", "enc_norm")] + [
        ("dec_layers", C.c_int32), ("dec_norm", C.c_int32), ("eps", C.c_float)]


class SfPixdecConfig(C.Structure):
    """sf_pixdec_config: the Mask2Former pixel decoder's fields as plain ints; per input level (by increasing stride) its channels, its
    stride and whether it enters the transformer encoder (norm 0 = "GN"; im2col_chunk_rows 0 = the library's default)."""
    _fields_ = [("num_levels", C.c_int32)] + [(n, C.c_int32 * 4) for n in ("channels", "strides", "in_transformer")] + [
        (n, C.c_int32) for n in ("conv_dim", "mask_dim", "nheads", "dim_feedforward", "enc_layers", "enc_n_points", "common_stride", "norm",
                                 "im2col_chunk_rows")]


class SfMaskdecConfig(C.Structure):
    """sf_maskdec_config: the Mask2Former transformer decoder's fields as plain ints (reid_layers -1 = the base class without
    ``reid_embed``, 0 = identity, n = an MLP of n layers)."""
    _fields_ = [(n, C.c_int32) for n in ("in_channels", "hidden_dim", "num_queries", "nheads", "dim_feedforward", "dec_layers", "mask_dim",
                                         "num_classes", "enforce_input_project", "pre_norm", "mask_classification", "reid_layers",
                                         "reid_hidden_dim")]


class SfMaskdecOutputs(C.Structure):
    """sf_maskdec_outputs: device addresses of one forward's outputs (0: not wanted)."""
    _fields_ = [(n, C.c_void_p) for n in ("pred_logits", "pred_masks", "pred_queries", "pred_embeds", "pred_bboxes", "aux_logits", "aux_masks",
                                          "aux_queries", "aux_embeds", "attn_masks")]


SF_OAD_MAX_CALL_STREAMS = 64
SF_STREAM_BLOB_KV1 = 0x31564B53


class SfCacheStreamMeta(C.Structure):
    """sf_cache_stream_meta: what a parked stream's blob is and where it may go back."""
    _fields_ = [("format", C.c_uint32)] + [(n, C.c_int32) for n in (
        "compute", "frames_seen", "frames_held", "max_frames", "policy", "H", "W", "layers", "hidden_size", "patches",
        "elem_bytes")] + [("packing", C.c_uint64), ("blob_bytes", C.c_uint64)]


class SfGemmDesc(C.Structure):
    """sf_gemm_desc: one forward GEMM with every field the forward sets (device addresses; 0: absent)."""
    _fields_ = [("split", C.c_int32)] + [(n, C.c_void_p) for n in ("a_hi", "a_lo", "w_hi", "w_lo", "bias")] + [
        (n, C.c_int32) for n in ("M", "N", "K", "epi", "act")] + [("alpha", C.c_float), ("resid", C.c_void_p), ("resid_mod", C.c_int32)] + [
        (n, C.c_void_p) for n in ("resid_hi", "resid_lo", "resid_lo2", "pos", "time_rows")] + [("Np", C.c_int32), ("Tn", C.c_int32)] + [
        (n, C.c_void_p) for n in ("out_f32", "out_hi", "out_lo", "out_lo2")] + [
        (n, C.c_int32) for n in ("ldc", "grp_rows", "grp_stride", "grp_off")] + [
        (n, C.c_void_p) for n in ("ln_stats_out", "ln_stats", "ln_s")] + [("ln_eps", C.c_float), ("ln_stats_wide", C.c_int32),
                                                                          ("ln_inkernel", C.c_int32)]


SF_GEMM_DISPATCH, SF_GEMM_SKINNY, SF_GEMM_TILE, SF_GEMM_PANEL, SF_GEMM_G256, SF_GEMM_G128, SF_GEMM_COLSPLIT = range(7)
SF_EPI_F32, SF_EPI_BF16, SF_EPI_ACT_BF16, SF_EPI_RESID_F32, SF_EPI_EMBED_F32 = range(5)


class NativeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"streamformer_hip error {code}: {msg}")
        self.code = code


# name -> (restype, argtypes): every symbol include/streamformer_hip.h declares
_P, _I, _F, _SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t
SIGNATURES = {
    "sf_create": (_I, [C.POINTER(SfConfig), _I, C.POINTER(_P)]),
    "sf_destroy": (None, [_P]),
    "sf_last_error": (C.c_char_p, []),
    "sf_abi_version": (_I, []),
    "sf_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I]),
    "sf_finalize_weights": (_I, [_P, _I, _I, _I]),
    "sf_missing_weights": (_I, [_P]),
    "sf_set_pixel_normalization": (_I, [_P, _P, _P, _I, _F]),
    "sf_workspace_bytes": (_I, [_P, _I, _I, _I, _I, C.POINTER(_SZ)]),
    "sf_forward": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_forward_profile": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _SZ, _P, C.POINTER(_F)]),
    "sf_forward_attentions": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_embed": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "sf_layers": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    "sf_post_head": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "sf_cache_create": (_I, [_P, _I, _I, _I, _I, C.POINTER(_P)]),
    "sf_cache_reset": (_I, [_P]),
    "sf_cache_length": (_I, [_P]),
    "sf_cache_stream_length": (_I, [_P, _I]),
    "sf_cache_reset_stream": (_I, [_P, _I]),
    "sf_cache_bytes": (_SZ, [_P]),
    "sf_cache_set_policy": (_I, [_P, _I]),
    "sf_cache_destroy": (None, [_P]),
    "sf_cache_stream_blob_bytes": (_I, [_P, _I, C.POINTER(_SZ)]),
    "sf_cache_export_stream": (_I, [_P, _P, _I, _P, _SZ, C.POINTER(SfCacheStreamMeta), _P]),
    "sf_cache_import_stream": (_I, [_P, _P, _I, _P, _SZ, C.POINTER(SfCacheStreamMeta), _P]),
    "sf_stream_workspace_bytes": (_I, [_P, _P, _I, C.POINTER(_SZ)]),
    "sf_forward_stream": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_forward_stream_slots": (_I, [_P, _P, _P, _I, _I, C.POINTER(_I), _I, _P, _P, _P, _P, _SZ, _P]),
    "sf_forward_stream_attentions": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_op_layernorm": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "sf_op_linear": (_I, [_P, _P, _P, _P, _F, _I, _P, _I, _I, _I, _I, _P, _SZ, _P]),
    "sf_op_linear_workspace_bytes": (_SZ, [_I, _I, _I]),
    "sf_op_gemm": (_I, [C.POINTER(SfGemmDesc), _I, C.POINTER(_I), _P]),
    "sf_op_attention": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "sf_op_attention_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sf_op_spatial_attention_plan": (_I, [_I, _I, _I, _I, _I, _I, _F, C.POINTER(_I), C.POINTER(_I), C.POINTER(_SZ)]),
    "sf_op_attention_cached": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, C.POINTER(_I), C.POINTER(_I), _P, _SZ, _P]),
    "sf_op_attention_cached_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I, _I, _I]),
    "sf_loss_workspace_bytes": (_SZ, [_I, _I]),
    "sf_retrieval_loss": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_localization_loss": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_grounding_loss": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_dense_text_logits": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "sf_mask_loss_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sf_mask_loss": (_I, [_P, _I, _I, _I, _I, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(_P), C.POINTER(C.c_int32), _I,
                          _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_dense_head_workspace_bytes": (_SZ, [_I, _I, _I]),
    "sf_dense_head_forward": (_I, [_P, _I, _I, _I, _F, C.POINTER(_P), _P, _P, _SZ, _P]),
    "sf_dense_head_backward": (_I, [_P, _I, _I, _I, _F, C.POINTER(_P), _P, C.POINTER(_P), _P, _SZ, _P]),
    "sf_trainer_create": (_I, [C.POINTER(SfConfig), _I, _I, _I, C.POINTER(_P)]),
    "sf_trainer_destroy": (None, [_P]),
    "sf_trainer_num_params": (_I, [_P]),
    "sf_trainer_param_info": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "sf_trainer_total_floats": (_I, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sf_trainer_num_stages": (_I, [_P]),
    "sf_trainer_stage_range": (_I, [_P, _I, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sf_trainer_sync_weights": (_I, [_P, _P, _P]),
    "sf_trainer_workspace_bytes": (_I, [_P, _I, _I, C.POINTER(_SZ)]),
    "sf_trainer_forward": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _SZ, _P]),
    "sf_trainer_backward": (_I, [_P, _P, _P, _P, _I, _I, _P, _SZ, _P]),
    "sf_trainer_adamw_step": (_I, [_P, _P, _P, _P, _P, _I, _F, _F, _F, _F, _F, _F, _P, _F, _I, _P]),
    "sf_trainer_set_drop_path": (_I, [_P, _P, _I, _I]),
    "sf_trainer_set_dropout": (_I, [_P, _F, _F, C.c_uint32]),
    "sf_trainer_set_nonfinite_guard": (_I, [_P, _P, _P]),
    "sf_trainer_set_extra_steps": (_I, [_P, C.POINTER(C.c_int32), _I]),
    "sf_trainer_grad_sumsq": (_I, [_P, _P, _P, _P]),
    "sf_op_wgrad": (_I, [_P, _I, _P, _I, _I, _I, _I, _F, _I, _P, _I, _P, _P]),
    "sf_op_attention_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_attention_bwd_hd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_layernorm_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _F, _P]),
    "sf_text_create": (_I, [C.POINTER(SfTextConfig), _I, C.POINTER(_P)]),
    "sf_text_destroy": (None, [_P]),
    "sf_text_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I]),
    "sf_text_finalize": (_I, [_P, _I]),
    "sf_text_missing_weights": (_I, [_P]),
    "sf_text_workspace_bytes": (_I, [_P, _I, _I, C.POINTER(_SZ)]),
    "sf_text_forward": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _SZ, _P]),
    "sf_text_forward_groups": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _SZ, _P]),
    "sf_op_text_attention": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "sf_op_text_pool": (_I, [_P, _I, _I, _I, _P, _P, _F, _P, _P, _I, _I, _P, _P, _P]),
    "sf_connector_create": (_I, [C.POINTER(SfConnectorConfig), _I, C.POINTER(_P)]),
    "sf_connector_destroy": (None, [_P]),
    "sf_connector_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I]),
    "sf_connector_finalize": (_I, [_P, _I]),
    "sf_connector_missing_weights": (_I, [_P]),
    "sf_connector_num_tokens": (_I, [_P, _I, _I, C.POINTER(C.c_int64)]),
    "sf_connector_workspace_bytes": (_I, [_P, _I, _I, C.POINTER(_SZ)]),
    "sf_connector_forward": (_I, [_P, _P, _I, _I, _P, _I, _P, _SZ, _P]),
    "sf_op_connector_pool": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P]),
    "sf_oad_create": (_I, [C.POINTER(SfOadConfig), _I, C.POINTER(_P)]),
    "sf_oad_destroy": (None, [_P]),
    "sf_oad_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I]),
    "sf_oad_finalize": (_I, [_P, _I]),
    "sf_oad_missing_weights": (_I, [_P]),
    "sf_oad_workspace_bytes": (_I, [_P, _I, C.POINTER(_SZ)]),
    "sf_oad_state_create": (_I, [_P, _I, C.POINTER(_P)]),
    "sf_oad_state_destroy": (None, [_P]),
    "sf_oad_state_reset": (_I, [_P, _I]),
    "sf_oad_state_fill": (_I, [_P, _I]),
    "sf_oad_state_copy": (_I, [_P, _I, _P, _I, _P]),
    "sf_oad_step": (_I, [_P, _P, C.POINTER(C.c_int32), _I, _P, _P, C.POINTER(C.c_int32), _P, _P, _I, _P, _SZ, _P]),
    "sf_op_oad_attention": (_I, [_P, _I, _P, _P, C.POINTER(C.c_int32), _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_msda_forward": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_msda_forward_fused": (_I, [_P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _I, _P, _I, _P, _I, _P,
                                      _I, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_msda_backward": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_adapter_dwconv_gelu": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sf_op_adapter_fuse": (_I, [_I, _P, C.c_longlong, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sf_op_adapter_dwconv_gelu_backward_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sf_op_adapter_dwconv_gelu_backward": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _SZ, _P]),
    "sf_op_adapter_fuse_backward": (_I, [_I, _P, _P, C.c_longlong, _I, _I, _I, _I, _P]),
    "sf_pixdec_create": (_I, [C.POINTER(SfPixdecConfig), _I, C.POINTER(_P)]),
    "sf_pixdec_destroy": (None, [_P]),
    "sf_pixdec_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I]),
    "sf_pixdec_finalize": (_I, [_P, _I]),
    "sf_pixdec_missing_weights": (_I, [_P]),
    "sf_pixdec_num_outputs": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "sf_pixdec_workspace_bytes": (_I, [_P, _I, C.POINTER(C.c_int32), _I, C.POINTER(_SZ)]),
    "sf_pixdec_forward": (_I, [_P, C.POINTER(_P), _I, C.POINTER(C.c_int32), _I, _P, C.POINTER(_P), _I, _P, _SZ, _P]),
    "sf_op_pixdec_nchw_to_planes": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "sf_op_pixdec_rows_to_nchw": (_I, [_P, C.c_longlong, _P, _I, _I, _I, _P]),
    "sf_op_pixdec_groupnorm": (_I, [_P, _P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "sf_op_pixdec_pos_ref": (_I, [_P, C.POINTER(C.c_int32), _I, _I, _I, _P, _P, _P]),
    "sf_op_pixdec_postln": (_I, [_P, _P, _P, _F, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sf_op_pixdec_im2col": (_I, [_P, _P, _I, _I, _I, _I, C.c_longlong, _I, _P, _P, _P]),
    "sf_op_pixdec_conv3x3_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "sf_op_pixdec_conv3x3": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _SZ, _P]),
    "sf_op_pixdec_groupnorm_backward_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sf_op_pixdec_groupnorm_backward": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _SZ, _P]),
    "sf_op_pixdec_upsample_backward": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sf_maskdec_create": (_I, [C.POINTER(SfMaskdecConfig), _I, C.POINTER(_P)]),
    "sf_maskdec_destroy": (None, [_P]),
    "sf_maskdec_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I]),
    "sf_maskdec_finalize": (_I, [_P, _I]),
    "sf_maskdec_missing_weights": (_I, [_P]),
    "sf_maskdec_workspace_bytes": (_I, [_P, _I, C.POINTER(C.c_int32), _I, _I, C.POINTER(_SZ)]),
    "sf_maskdec_forward": (_I, [_P, C.POINTER(_P), _P, _I, C.POINTER(C.c_int32), _I, _I, C.POINTER(SfMaskdecOutputs), _P, _SZ, _P]),
    "sf_op_maskdec_attention": (_I, [_P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_maskattn_forward": (_I, [_P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_maskattn_backward": (_I, [_P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sf_op_maskattn_pack": (_I, [_P, _P, C.c_longlong, _I, _P]),
    "sf_op_maskdec_boxes": (_I, [_P, _P, _I, _I, _I, _P]),
    "sf_op_masklogits_forward": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "sf_op_masklogits_backward_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sf_op_masklogits_backward": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _SZ, _P]),
    "sf_op_maskdec_mask_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sf_op_maskdec_mask": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "sf_op_vis_scores": (_I, [_P, C.c_longlong, _I, _P, _P, _P, _P]),
    "sf_op_vis_pack_masks": (_I, [_P, C.c_longlong, _I, _P, _P, _P]),
    "sf_op_vis_mask_iou": (_I, [_P, _I, _I, _I, _P, _P]),
    "sf_op_vis_postprocess_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sf_op_vis_postprocess": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_op_seg_semantic": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "sf_op_seg_panoptic_argmax": (_I, [_P, _P, _P, _I, _I, _F, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "sf_op_seg_panoptic_relabel": (_I, [_P, _P, _I, C.c_longlong, _P, _P]),
    "sf_op_crit_costs_workspace_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "sf_op_crit_costs": (_I, [C.POINTER(_P), C.POINTER(_P), _I, _I, _I, _I, _I, _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32),
                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, _I, _I, _F, _F, _F, _P, _P, _SZ, _P]),
    "sf_op_crit_losses_capacity": (_I, []),
    "sf_op_crit_losses_workspace_bytes": (_SZ, [_I]),
    "sf_op_crit_losses": (_I, [C.POINTER(_P), _I, _I, _I, _I, _I, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                               C.POINTER(C.c_int32), _P, C.POINTER(C.c_int32), _I, _P, _P, _I, _I, _I, _F, _P, _I, _P, _P, _P, _P, _SZ, _P]),
    "sf_op_crit_losses_backward": (_I, [C.POINTER(_P), _I, _I, _I, _I, _I, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), _P, _I, _P, _P, _I, _F, _P, _P, _P]),
    "sf_op_crit_class_loss_workspace_bytes": (_SZ, [_I, _I, _I]),
    "sf_op_crit_class_loss": (_I, [C.POINTER(_P), _I, _I, _I, _I, _P, _I, C.POINTER(_P), C.POINTER(C.c_int32), _P, _P, _I, _P, _P, _P, _SZ,
                                   _P]),
    "sf_op_clp_tracks": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _P]),
    "sf_op_clp_items": (_I, [_P, _I, _I, _P, _I, _I, _P, _I, _P, _I, _I, _P, _P, _P]),
    "sf_op_clp_backward_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "sf_op_clp_backward": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _I, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    "sf_reload_switches": (None, []),
    "sf_switch_info": (C.c_char_p, [_I, _I]),
    "sf_bench_launch_floor": (_I, [_I, _I, _I, _P, C.POINTER(_F)]),
    "sf_bench_gemm": (_I, [_P, _I, _I, _I, _P, _SZ, _P, C.POINTER(_F), C.POINTER(C.c_double)]),
    "sf_bench_attention": (_I, [_P, _I, _I, _I, _I, _P, _SZ, _P, C.POINTER(_F), C.POINTER(C.c_double),
                                C.POINTER(C.c_double)]),
}


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python streamformer_amd/build.py` "
            "(hipcc --offload-arch=gfx950).  There is no non-HIP fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{LIB_PATH} does not export {name} (stale build? run "
                              "`python streamformer_amd/build.py`)") from e
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(code: int) -> None:
    if code != SF_OK:
        raise NativeError(code, (lib.sf_last_error() or b"").decode(errors="replace"))


def ptr(t) -> int:
    """Device/host address of a tensor (0 for None)."""
    return 0 if t is None else t.data_ptr()


def weights_token(device, tensors):
    """What a packed handle was made from: the device and every tensor's address and in-place version counter."""
    return (device, tuple((t.data_ptr(), t._version) for t in tensors))


def load_tensors(handle, load_fn, items, dtype_of=None) -> None:
    """Stage ``(key, tensor)`` pairs through a ``*_load_tensor`` entry point from contiguous host copies.  ``dtype_of`` maps a torch
    dtype that the entry point takes as it is to its SF_* code (None: convert); without it everything goes as fp32."""
    for k, p in items:
        t = p.detach().to("cpu").contiguous()
        code = dtype_of(t.dtype) if dtype_of is not None else None
        if code is None:
            t, code = t.float(), SF_F32
        shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
        check(load_fn(handle, k.encode(), t.data_ptr(), code, shape, t.dim()))


_COMPUTE_MODES = {"bf16": SF_COMPUTE_BF16, "bfloat16": SF_COMPUTE_BF16, torch.bfloat16: SF_COMPUTE_BF16,
                  "bf16x3": SF_COMPUTE_BF16X3, "fp32": SF_COMPUTE_BF16X3, "float32": SF_COMPUTE_BF16X3, torch.float32: SF_COMPUTE_BF16X3}


def compute_mode(value) -> int:
    """The SF_COMPUTE_* code of a module's ``compute_dtype`` argument."""
    try:
        return _COMPUTE_MODES[value]
    except KeyError:
        raise ValueError(f"compute_dtype must be one of 'bf16' (throughput) or 'fp32'/'bf16x3' (accurate), got {value!r}") from None


class OwnedHandle(C.c_void_p):
    """A native handle that is not rebuilt from weights (a probe, a detector state, a stream cache).  It IS the ``c_void_p``: its
    ``*_create`` fills it through ``C.byref`` and every entry point takes it as it is.  Destroyed once, by ``release()`` or when it is
    collected; false afterwards; never copied."""

    def __init__(self, destroy, noun: str):
        super().__init__()
        self._destroy, self._noun = destroy, noun

    def release(self) -> None:
        h, self.value = self.value, None
        if h:
            self._destroy(h)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    __hash__ = object.__hash__             # (c_void_p is unhashable; PackedHandle.dependents is a WeakSet)

    def __reduce_ex__(self, protocol):
        raise TypeError(f"a {self._noun} is device memory of one native handle and cannot be copied or pickled: make a new one")


def _held(fn):
    """How an owner keeps a callable.  A bound method weakly: the module owns the PackedHandle, and a strong reference back would leave
    the native memory to the cycle collector instead of freeing it with the module's last reference.  A library entry point by name
    (``_strong`` looks it up): ctypes function pointers neither pickle nor deep-copy."""
    if isinstance(fn, lib._FuncPtr):
        return fn.__name__
    return weakref.WeakMethod(fn) if inspect.ismethod(fn) else fn


def _strong(fn):
    return getattr(lib, fn) if isinstance(fn, str) else fn() if isinstance(fn, weakref.WeakMethod) else fn


class PackedHandle:
    """The native state one module builds from its tensors: the packed handle(s), the token of what they were packed from, the
    workspaces.  ``create(device_index[, key]) -> c_void_p``, ``load_tensor`` (a ``*_load_tensor`` entry point), ``finalize(handle)`` and
    ``destroy(handle)`` are the family's calls; ``on_release()`` runs before handles are destroyed, while the module lives; ``noun`` (or
    the whole ``refusal``) words the error for a module that is not on the GPU; ``dtype_of`` is ``load_tensors``'s.  ``dependents`` are
    OwnedHandles made against a packed handle (stream caches): released before it, whoever releases it.  A copy or a pickle of an owner
    is an empty owner of the same family, so the callables are bound methods of the module, library entry points or module-level
    functions; ``destroy`` must not be a method of the module, which may be gone when it is called."""

    def __init__(self, create=None, load_tensor=None, finalize=None, destroy=None, noun: str = "module", on_release=None, dtype_of=None,
                 refusal: str = None):
        self._family = tuple(_held(f) for f in (create, load_tensor, finalize, destroy, on_release, dtype_of))
        self._noun, self._refusal = noun, refusal
        self.handles: dict = {}             # key -> c_void_p; the one handle of most modules is under None
        self.token = None
        self.workspaces: dict = {}          # key -> uint8 tensor; dropped with the handles
        self.dependents = weakref.WeakSet()

    def get(self, device, token, items, key=None):
        """The handle of ``key``, packed from ``items`` ((name, tensor) pairs, or a callable that lists them) unless the handles held
        were made from ``token`` already.  Another token destroys every handle held and drops the workspaces first."""
        if device.type != "cuda":
            raise RuntimeError(self._refusal or f"the {self._noun} runs on the MI355X: move the module with .to('cuda') (there is no CPU fallback)")
        if token != self.token:
            self.release()
            self.token = token
        h = self.handles.get(key)
        if h is None:
            create, load_tensor, finalize, destroy, _, dtype_of = map(_strong, self._family)
            h = create(device.index or 0) if key is None else create(device.index or 0, key)
            try:
                load_tensors(h, load_tensor, items() if callable(items) else items, dtype_of)
                with torch.cuda.device(device):
                    finalize(h)
            except BaseException:
                destroy(h)
                raise
            self.handles[key] = h
        return h

    def workspace(self, nbytes: int, device, key=None) -> torch.Tensor:
        """The grow-only byte buffer of ``key``: the one held when it is large enough and on ``device``, else a new one."""
        ws = self.workspaces.get(key)
        if ws is None or ws.numel() < nbytes or ws.device != device:
            self.workspaces.pop(key, None)       # before the new one is made: both need not fit at once
            ws = self.workspaces[key] = scratch(nbytes, device)
        return ws

    def release(self) -> None:
        handles, self.handles, self.token = self.handles, {}, None
        self.workspaces.clear()
        if handles:
            on_release, destroy = _strong(self._family[4]), _strong(self._family[3])
            if on_release is not None:
                on_release()
            for d in list(self.dependents):
                d.release()
            for h in handles.values():
                destroy(h)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def __reduce_ex__(self, protocol):
        family = tuple(f() if isinstance(f, weakref.WeakMethod) else f for f in self._family)      # entry points stay names
        return (PackedHandle, family[:4] + (self._noun,) + family[4:] + (self._refusal,))


def current_stream_handle(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


_ABSENT = object()
WORKSPACE_FLOOR = 256      # bytes: the least any byte buffer handed to the library has, so that its address is never null


# Written out at their call sites, not through ``launch``: sf_forward_profile and the sf_bench_* family (a result pointer follows the
# stream), and a call whose code the caller reads instead of raising (the refusal probes).  Everything else that takes a stream goes
# through ``launch``.
def launch(device, fn, *args, workspace=_ABSENT) -> None:
    """``fn(*args[, workspace address, workspace bytes], stream)`` with ``device`` current and its current stream last; raises NativeError
    on a non-zero code.  ``fn`` is the entry point itself (``nat.lib.sf_op_x`` at the call site); ``workspace`` is a byte tensor or
    None (0, 0)."""
    if workspace is not _ABSENT:
        args += (ptr(workspace), 0 if workspace is None else workspace.numel())
    if device.index in (None, torch.cuda.current_device()):      # current already (a one-GPU process, a caller's own guard): no guard entry
        check(fn(*args, current_stream_handle(device)))
    else:
        with torch.cuda.device(device):
            check(fn(*args, current_stream_handle(device)))


def sized(fn, *args) -> int:
    """What a sizer that answers through a trailing ``size_t*`` wrote."""
    n = C.c_size_t()
    check(fn(*args, C.byref(n)))
    return n.value


def scratch(nbytes: int, device) -> torch.Tensor:
    """A one-shot byte buffer of at least ``nbytes``; the caller keeps it until its launch is enqueued."""
    return torch.empty(max(int(nbytes), WORKSPACE_FLOOR), dtype=torch.uint8, device=device)


def ptr_array(tensors):
    """ctypes array of the tensors' addresses (None -> 0), at least one element long."""
    return (C.c_void_p * max(len(tensors), 1))(*[ptr(t) for t in tensors])


def i32_array(values):
    """ctypes int32 array of the values, at least one element long."""
    return (C.c_int32 * max(len(values), 1))(*[int(v) for v in values])
