"""ctypes binding of libconsolver_hip.so (the C ABI in include/consolver_hip.h).

There is NO fallback: if the library is missing or a call fails, a
``RuntimeError`` is raised.  The product never computes on the CPU.
"""
import ctypes as C
import os

import torch

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CONSOLVER_HIP_LIB") or os.path.join(PKG, "libconsolver_hip.so")   # override: A/B builds in tools/

CS_F32, CS_F16, CS_BF16, CS_U8 = 0, 1, 2, 3
CS_MAX_ORDER = 8
CS_LIN_MAX_TERMS = 4
_DT = {torch.float32: CS_F32, torch.float16: CS_F16, torch.bfloat16: CS_BF16}


class CsFactorNet(C.Structure):
    _fields_ = [("w0", C.c_void_p), ("b0", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p),
                ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("in_dim", C.c_int), ("hidden", C.c_int), ("action_dims", C.c_int), ("num_actions", C.c_int),
                ("input_scale", C.c_float), ("inv_temperature", C.c_float)]


class CsStepArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("eps_text", C.c_void_p), ("eps_uncond", C.c_void_p), ("guidance", C.c_float),
                ("hist", C.c_void_p * CS_MAX_ORDER), ("m", C.c_int), ("order_dim", C.c_int), ("scaler_dim", C.c_int),
                ("actions", C.c_void_p), ("actions_stride", C.c_int), ("B", C.c_int), ("elems", C.c_int64),
                ("io_dtype", C.c_int), ("out_dtype", C.c_int), ("x_out", C.c_void_p), ("eps_out", C.c_void_p),
                ("sqrt_at", C.c_float), ("sqrt_1mat", C.c_float), ("sqrt_ap", C.c_float), ("sqrt_1map", C.c_float),
                ("v_prediction", C.c_int), ("dt", C.c_float), ("x_is_f32", C.c_int), ("x_out_lp", C.c_void_p), ("lp_dtype", C.c_int)]


class CsDpmStepArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("eps_text", C.c_void_p), ("eps_uncond", C.c_void_p), ("guidance", C.c_float), ("m_prev", C.c_void_p),
                ("B", C.c_int), ("elems", C.c_int64), ("io_dtype", C.c_int), ("out_dtype", C.c_int), ("x_is_f32", C.c_int),
                ("x_out", C.c_void_p), ("m_out", C.c_void_p), ("x_out_lp", C.c_void_p), ("lp_dtype", C.c_int),
                ("conv_x", C.c_float), ("conv_e", C.c_float), ("cx", C.c_float), ("c0", C.c_float), ("c1", C.c_float)]


class CsLinStepArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("eps_text", C.c_void_p), ("eps_uncond", C.c_void_p), ("guidance", C.c_float), ("x_base", C.c_void_p),
                ("hist", C.c_void_p * (CS_LIN_MAX_TERMS - 1)), ("terms", C.c_int), ("B", C.c_int), ("elems", C.c_int64), ("io_dtype", C.c_int),
                ("out_dtype", C.c_int), ("x_is_f32", C.c_int), ("x_out", C.c_void_p), ("m_out", C.c_void_p), ("x_out_lp", C.c_void_p),
                ("lp_dtype", C.c_int), ("conv_x", C.c_float), ("conv_e", C.c_float), ("cx", C.c_float), ("c", C.c_float * CS_LIN_MAX_TERMS)]


class CsUnipcStepArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("eps_text", C.c_void_p), ("eps_uncond", C.c_void_p), ("guidance", C.c_float), ("x_last", C.c_void_p),
                ("m_prev0", C.c_void_p), ("m_prev1", C.c_void_p), ("B", C.c_int), ("elems", C.c_int64), ("io_dtype", C.c_int), ("out_dtype", C.c_int),
                ("x_is_f32", C.c_int), ("use_corr", C.c_int), ("x_out", C.c_void_p), ("m_out", C.c_void_p), ("x_last_out", C.c_void_p),
                ("x_out_lp", C.c_void_p), ("lp_dtype", C.c_int),
                ("conv_x", C.c_float), ("conv_e", C.c_float), ("a_x", C.c_float), ("a_0", C.c_float), ("a_1", C.c_float), ("a_n", C.c_float),
                ("p_x", C.c_float), ("p_0", C.c_float), ("p_1", C.c_float)]


class CsFmStepArgs(C.Structure):
    _fields_ = [("x_base", C.c_void_p), ("v2", C.c_void_p), ("v1", C.c_void_p), ("c", C.c_float), ("B", C.c_int), ("elems", C.c_int64),
                ("io_dtype", C.c_int), ("out_dtype", C.c_int), ("x_is_f32", C.c_int), ("x_out", C.c_void_p)]


class CsFluxConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("num_layers", C.c_int), ("num_single_layers", C.c_int), ("num_heads", C.c_int),
                ("head_dim", C.c_int), ("joint_attention_dim", C.c_int), ("pooled_projection_dim", C.c_int),
                ("guidance_embeds", C.c_int), ("axes_dims_rope", C.c_int * 3), ("dtype", C.c_int)]


class CsUNetConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("block_out_channels", C.c_int * 4),
                ("layers_per_block", C.c_int), ("num_heads", C.c_int), ("cross_attention_dim", C.c_int),
                ("norm_num_groups", C.c_int), ("sample_size", C.c_int), ("ctx_len", C.c_int),
                ("down_has_attn", C.c_int * 4), ("up_has_attn", C.c_int * 4)]


class CsVaeConfig(C.Structure):
    _fields_ = [("latent_channels", C.c_int), ("out_channels", C.c_int), ("block_out_channels", C.c_int * 4),
                ("layers_per_block", C.c_int), ("norm_num_groups", C.c_int), ("sample_size", C.c_int), ("use_post_quant_conv", C.c_int),
                ("with_encoder", C.c_int), ("use_quant_conv", C.c_int)]


class CsClipConfig(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_hidden_layers", C.c_int),
                ("num_attention_heads", C.c_int), ("max_position_embeddings", C.c_int), ("layer_norm_eps", C.c_float)]


class CsVitConfig(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("num_hidden_layers", C.c_int), ("num_attention_heads", C.c_int), ("mlp_ratio", C.c_int),
                ("image_size", C.c_int), ("patch_size", C.c_int), ("layer_norm_eps", C.c_float), ("resize_shortest_edge", C.c_int),
                ("crop_size", C.c_int), ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3), ("rescale_factor", C.c_double)]


class CsClipVisionConfig(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_hidden_layers", C.c_int), ("num_attention_heads", C.c_int),
                ("image_size", C.c_int), ("patch_size", C.c_int), ("projection_dim", C.c_int), ("layer_norm_eps", C.c_float),
                ("resize_shortest_edge", C.c_int), ("crop_size", C.c_int), ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3),
                ("rescale_factor", C.c_double)]


class CsDepthConfig(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("num_hidden_layers", C.c_int), ("num_attention_heads", C.c_int), ("mlp_ratio", C.c_int),
                ("image_size", C.c_int), ("patch_size", C.c_int), ("layer_norm_eps", C.c_float), ("out_indices", C.c_int * 4),
                ("neck_hidden_sizes", C.c_int * 4), ("fusion_hidden_size", C.c_int), ("head_hidden_size", C.c_int), ("max_depth", C.c_float),
                ("size", C.c_int), ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3), ("rescale_factor", C.c_double)]


class CsSegConfig(C.Structure):
    _fields_ = [("hidden_sizes", C.c_int * 4), ("depths", C.c_int * 4), ("num_attention_heads", C.c_int * 4), ("sr_ratios", C.c_int * 4), ("mlp_ratio", C.c_int),
                ("decoder_hidden_size", C.c_int), ("num_labels", C.c_int), ("size", C.c_int), ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3),
                ("rescale_factor", C.c_double)]


class CsIncepConfig(C.Structure):
    _fields_ = [("image_size", C.c_int), ("num_classes", C.c_int), ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3), ("rescale_factor", C.c_double)]


class CsFidConfig(C.Structure):
    _fields_ = [("image_mean", C.c_float * 3), ("image_std", C.c_float * 3)]


class CsGemm2Problem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("M", C.c_int), ("K", C.c_int), ("w", C.c_void_p), ("bias", C.c_void_p), ("N", C.c_int),
                ("res", C.c_void_p), ("gate", C.c_void_p), ("gate_stride", C.c_long), ("rows_per_sample", C.c_int), ("act", C.c_int),
                ("out", C.c_void_p), ("ldc", C.c_long), ("col_off", C.c_int)]


class CsGemm2Addressing(C.Structure):
    _fields_ = [("lda", C.c_long), ("a_seg_rows", C.c_int), ("a_seg_stride", C.c_int), ("a_row_off", C.c_long),
                ("c_seg_rows", C.c_int), ("c_seg_stride", C.c_int), ("c_row_off", C.c_long), ("res_lo", C.c_void_p), ("out_lo", C.c_void_p)]


# every symbol declared in include/consolver_hip.h: name -> (restype, argtypes)
SYMBOLS = {
    "cs_abi_version": (C.c_int, []),
    "cs_error_string": (C.c_char_p, [C.c_int]),
    "cs_last_error": (C.c_char_p, []),
    "cs_target_arch": (C.c_char_p, []),
    "cs_factor_probs": (C.c_int, [C.POINTER(CsFactorNet), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_cosine_features": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_cosine_features_cfg": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_float, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "cs_sample_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_gather_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_action_probs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_step_masks": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_stack_history": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_lms_ddim_step": (C.c_int, [C.POINTER(CsStepArgs), C.c_void_p]),
    "cs_lms_euler_step": (C.c_int, [C.POINTER(CsStepArgs), C.c_void_p]),
    "cs_dpm_multistep_step": (C.c_int, [C.POINTER(CsDpmStepArgs), C.c_void_p]),
    "cs_linear_step": (C.c_int, [C.POINTER(CsLinStepArgs), C.c_void_p]),
    "cs_unipc_step": (C.c_int, [C.POINTER(CsUnipcStepArgs), C.c_void_p]),
    "cs_fm_general_step": (C.c_int, [C.POINTER(CsFmStepArgs), C.c_void_p]),
    "cs_true_cfg_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "cs_psnr_workspace_bytes": (C.c_size_t, [C.c_int]),
    "cs_image_psnr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_void_p]),
    "cs_image_psnr_bcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_int64]),
    "cs_gather_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_ppo_advantages": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_ppo_advantages_baseline": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_ppo_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                              C.c_void_p]),
    "cs_policy_param_count": (C.c_size_t, [C.POINTER(CsFactorNet)]),
    "cs_policy_workspace_bytes": (C.c_size_t, [C.POINTER(CsFactorNet), C.c_int]),
    "cs_ppo_policy_grads": (C.c_int, [C.POINTER(CsFactorNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_clip_grad_norm": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "cs_adamw_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_float,
                                C.c_float, C.c_float, C.c_void_p]),
    "cs_clip_create": (C.c_int, [C.POINTER(CsClipConfig), C.POINTER(C.c_void_p)]),
    "cs_clip_destroy": (None, [C.c_void_p]),
    "cs_clip_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "cs_clip_num_weights": (C.c_int, [C.c_void_p]),
    "cs_clip_weight_name": (C.c_char_p, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "cs_clip_finalize": (C.c_int, [C.c_void_p]),
    "cs_clip_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "cs_clip_flops": (C.c_double, [C.c_void_p, C.c_int, C.c_int]),
    "cs_clip_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_cosine_reward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "cs_depth_normalized_maps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # images of any aspect ratio (csrc/depth_hw.cpp, csrc/segformer.cpp)
    "cs_depth_processed_size": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "cs_depth_preprocess_workspace_bytes_hw": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "cs_depth_preprocess_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_depth_workspace_bytes_hw": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "cs_depth_flops_hw": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "cs_depth_forward_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_depth_normalized_maps_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_depth_position_table": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "cs_seg_preprocess_hw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_vae_create": (C.c_int, [C.POINTER(CsVaeConfig), C.POINTER(C.c_void_p)]),
    "cs_vae_destroy": (None, [C.c_void_p]),
    "cs_vae_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "cs_vae_num_weights": (C.c_int, [C.c_void_p]),
    "cs_vae_weight_name": (C.c_char_p, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "cs_vae_finalize": (C.c_int, [C.c_void_p]),
    "cs_vae_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "cs_vae_flops": (C.c_double, [C.c_void_p, C.c_int]),
    "cs_vae_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                C.c_void_p]),
    "cs_vae_encode_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "cs_vae_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_unet_create": (C.c_int, [C.POINTER(CsUNetConfig), C.POINTER(C.c_void_p)]),
    "cs_unet_destroy": (None, [C.c_void_p]),
    "cs_unet_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
    "cs_unet_num_weights": (C.c_int, [C.c_void_p]),
    "cs_unet_weight_name": (C.c_char_p, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "cs_unet_finalize": (C.c_int, [C.c_void_p]),
    "cs_unet_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "cs_unet_flops": (C.c_double, [C.c_void_p, C.c_int]),
    "cs_unet_flops_executed": (C.c_double, [C.c_void_p, C.c_int, C.c_int]),
    "cs_unet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "cs_unet_set_residual_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "cs_unet_get_residual_precision": (C.c_int, [C.c_void_p]),
    "cs_unet_calibrate_ln_fold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_float, C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_float)]),
    "cs_unet_set_ln_unfold_mask": (C.c_int, [C.c_void_p, C.c_uint]),
    "cs_unet_get_ln_unfold_mask": (C.c_uint, [C.c_void_p]),
    "cs_unet_set_output_dtype": (C.c_int, [C.c_void_p, C.c_int]),
    "cs_unet_get_output_dtype": (C.c_int, [C.c_void_p]),
    "cs_unet_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "cs_unet_profile_entries": (C.c_int, [C.c_void_p]),
    "cs_unet_profile_entry": (C.c_char_p, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "cs_flux_create": (C.c_int, [C.POINTER(CsFluxConfig), C.POINTER(C.c_void_p)]),
    "cs_flux_destroy": (None, [C.c_void_p]),
    "cs_flux_num_weights": (C.c_int, [C.c_void_p]),
    "cs_flux_weight_name": (C.c_char_p, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "cs_flux_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_int]),
    "cs_flux_finalize": (C.c_int, [C.c_void_p]),
    "cs_flux_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "cs_flux_flops": (C.c_double, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "cs_flux_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_flux_set_residual_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "cs_flux_get_residual_precision": (C.c_int, [C.c_void_p]),
    "cs_flux_set_output_dtype": (C.c_int, [C.c_void_p, C.c_int]),
    "cs_flux_get_output_dtype": (C.c_int, [C.c_void_p]),
    "cs_flux_forward_joint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_flux_forward_joint_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # include/consolver_hip_ops.h
    "cs_op_gemm2_x2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_ln_modulate_x2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int, C.c_void_p]),
    "cs_op_gemm2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long,
                              C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]),
    "cs_op_attention_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "cs_op_attention_ws": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_gemm2_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_gemm2_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "cs_op_gemm2_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_qk_norm_rope": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]),
    "cs_op_small_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cs_op_ln_modulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_float,
                                    C.c_int, C.c_void_p]),
    "cs_op_sinusoid_f32": (C.c_int, [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_add3_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cs_op_cast_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "cs_op_planes_to_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "cs_op_attention_causal": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "cs_op_rms_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "cs_op_gated_mul": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "cs_op_embed_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "cs_op_attention_bias": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p]),
    "cs_op_attention_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "cs_op_conv2d": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "cs_op_geglu_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_attention": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "cs_op_conv_out": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cs_op_group_norm_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "cs_op_group_norm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_xattn_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "cs_op_conv2d_x2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_linear_x2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_ln_fold_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_linear_ln": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_row_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_row_stats_lo8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_conv_up_fold_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "cs_op_conv_up_sub": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_ln_dc_ratio": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "cs_op_linear_lo8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_size_t, C.c_void_p]),
    "cs_op_xattn_block_lo8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_group_norm_x2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_layer_norm_x2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "cs_op_xattn_block_x2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_unet_set_tuning": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "cs_unet_clear_tuning": (C.c_int, [C.c_void_p]),
    "cs_set_tuning": (C.c_int, [C.c_char_p, C.c_int]),
    "cs_get_tuning": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "cs_reset_tuning": (C.c_int, []),
    "cs_op_conv2d_gn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "cs_op_group_norm_pre": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_debug_trace_read": (C.c_int, [C.c_void_p, C.c_size_t]),
    "cs_debug_attn_trace_read": (C.c_int, [C.c_void_p, C.c_size_t]),
    "cs_debug_igemm_last_route": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "cs_op_layer_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "cs_op_clipv_tokens_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cs_op_clipv_head": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_dpt_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "cs_op_dpt_bilinear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_dpt_pixel_shuffle": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_dpt_pixel_shuffle_hw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_vit_pos_interp": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_dpt_head": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "cs_op_dpt_bicubic": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_dpt_minmax_normalize": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "cs_seg_masks": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "cs_seg_set_stage_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "cs_seg_agreement": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "cs_op_seg_dwconv_gelu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_seg_im2col": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_seg_patchify": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_seg_bilinear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "cs_op_seg_argmax": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_seg_logits": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_seg_relu": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "cs_incep_set_stage_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "cs_op_incep_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "cs_op_incep_maxpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "cs_op_incep_avgpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_incep_head": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_fid_avgpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_fid_maxpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_time_embedding": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_rowvec_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "cs_op_conv_in": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_op_embed_tokens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "cs_op_quick_gelu": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "cs_op_gelu_erf": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "cs_op_row_softmax": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p]),
    "cs_op_latent_to_nhwc64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "cs_op_pixel_linear": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "cs_op_pixel_affine": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "cs_op_conv_down": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "cs_op_group_norm_workspace_splits": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "cs_op_group_norm_splits": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "cs_fid_stats_accumulate":(C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cs_fid_stats_finalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# the image-tower handle families (csrc/image_tower.h) declare the same 13 entry points, each over its own config struct
for _prefix, _config in (("vit", CsVitConfig), ("clipv", CsClipVisionConfig), ("depth", CsDepthConfig), ("seg", CsSegConfig), ("incep", CsIncepConfig),
                         ("fid", CsFidConfig)):
    SYMBOLS.update({
        f"cs_{_prefix}_create": (C.c_int, [C.POINTER(_config), C.POINTER(C.c_void_p)]),
        f"cs_{_prefix}_destroy": (None, [C.c_void_p]),
        f"cs_{_prefix}_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int]),
        f"cs_{_prefix}_num_weights": (C.c_int, [C.c_void_p]),
        f"cs_{_prefix}_weight_name": (C.c_char_p, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
        f"cs_{_prefix}_finalize": (C.c_int, [C.c_void_p]),
        f"cs_{_prefix}_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
        f"cs_{_prefix}_flops": (C.c_double, [C.c_void_p, C.c_int]),
        f"cs_{_prefix}_patch_cols": (C.c_int, [C.c_void_p]),
        f"cs_{_prefix}_num_tokens": (C.c_int, [C.c_void_p]),
        f"cs_{_prefix}_preprocess_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
        f"cs_{_prefix}_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_void_p]),
        f"cs_{_prefix}_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    })

_lib = None


def lib():
    """Load (once) and return the bound library; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -m consolver_amd.build`). There is no CPU fallback.")
    l = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            f = getattr(l, name)
        except AttributeError as e:
            raise RuntimeError(f"libconsolver_hip.so does not export {name}") from e
        f.restype = res
        f.argtypes = args
    if l.cs_abi_version() != 2:
        raise RuntimeError("libconsolver_hip.so ABI version mismatch")
    _lib = l
    try:
        apply_env_tuning()
    except Exception:
        _lib = None          # a malformed CS_TUNE raises on EVERY call, not only the first (the library must not come up with the remaining knobs silently unapplied)
        raise
    return l


def apply_env_tuning():
    """CS_TUNE="key=value,..." applies kernel-selection knobs (cs_set_tuning): A/B runs of tests and tools without code changes.  Called at load
    time and by reset_tuning()."""
    for kv in os.environ.get("CS_TUNE", "").split(","):
        if "=" in kv:
            k, v = kv.split("=", 1)
            if _lib.cs_set_tuning(k.strip().encode(), int(v)) != 0:
                raise RuntimeError(f"CS_TUNE: {_lib.cs_last_error().decode()}")


def reset_tuning():
    """every knob back to its default (then CS_TUNE re-applied): what tests/conftest.py runs after each test."""
    lib().cs_reset_tuning()
    apply_env_tuning()


def check(code):
    if code != 0:
        l = lib()
        raise RuntimeError(f"libconsolver_hip: {l.cs_error_string(code).decode()}: {l.cs_last_error().decode()}")


# ---- the weight-loading protocol every model handle shares: cs_<prefix>_num_weights / _weight_name / _set_weight / _finalize / _destroy ----
def manifest(prefix, handle, cap=4):
    """[(name, shape)] in the handle's state-dict naming; ``cap``: the dims cs_<prefix>_weight_name writes (2 for flux)."""
    l = lib()
    out, shape, nd = [], (C.c_int64 * cap)(), C.c_int()
    for i in range(getattr(l, f"cs_{prefix}_num_weights")(handle)):
        name = getattr(l, f"cs_{prefix}_weight_name")(handle, i, shape, C.byref(nd)).decode()
        out.append((name, tuple(shape[k] for k in range(nd.value))))
    return out


def load_float_weights(prefix, handle, state_dict, device, strict=True):
    """every tensor of the manifest from ``state_dict`` as host fp32 through cs_<prefix>_set_weight, then cs_<prefix>_finalize on ``device``."""
    l = lib()
    want = dict(manifest(prefix, handle))
    missing = [k for k in want if k not in state_dict]
    if missing and strict:
        raise KeyError(f"missing {len(missing)} tensors, e.g. {missing[:3]}")
    set_weight = getattr(l, f"cs_{prefix}_set_weight")
    for name, shape in want.items():
        t = state_dict[name].detach().to("cpu", torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: shape {tuple(t.shape)} != {shape}")
        sh = (C.c_int64 * len(shape))(*shape)
        check(set_weight(handle, name.encode(), C.c_void_p(t.data_ptr()), sh, len(shape)))
    torch.cuda.set_device(device)
    check(getattr(l, f"cs_{prefix}_finalize")(handle))


def destroy(prefix, obj):
    """__del__ of a handle-owning object: cs_<prefix>_destroy of ``obj._h``, once; never raises (interpreter shutdown)."""
    try:
        if getattr(obj, "_h", None):
            getattr(lib(), f"cs_{prefix}_destroy")(obj._h)
            obj._h = None
    except Exception:
        pass


def dtype_code(dt):
    try:
        return _DT[dt]
    except KeyError:
        raise TypeError(f"unsupported dtype {dt}; expected float32/float16/bfloat16")


def require_cuda(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(
            f"{name} must be a CUDA (ROCm) tensor: consolver_amd runs only on the MI355X HIP path; "
            "the CPU restatement lives in oracle/ and is test infrastructure, not a fallback.")
    return t


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
