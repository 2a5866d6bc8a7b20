"""ctypes binding of libhedit_hip.so (include/hedit.h).  Fails loudly if the library is absent."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HEDIT_STORAGE=f16 selects the half-storage build of the same kernels (`python h-edit_amd/build.py --f16`, csrc/common.h): same
# MFMA rate, the eps error of the SD UNet against fp32 1.7e-3 instead of bfloat16's 1.2e-2.  One storage format per process,
# decided before the library is first used.  Default and every benchmark figure: bfloat16 (BASELINE configs[1]).
STORAGE = os.environ.get("HEDIT_STORAGE", "bf16").lower()
if STORAGE not in ("bf16", "f16"):
    raise ValueError(f"HEDIT_STORAGE must be bf16 or f16, not {STORAGE!r}")
LIB_PATH = os.path.join(_HERE, "libhedit_hip_f16.so" if STORAGE == "f16" else "libhedit_hip.so")
HEDIT_MAX_LEVELS = 8


class UnetCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("sample_size", C.c_int),
                ("n_levels", C.c_int),
                ("block_out_channels", C.c_int * HEDIT_MAX_LEVELS),
                ("down_has_attn", C.c_int * HEDIT_MAX_LEVELS),
                ("up_has_attn", C.c_int * HEDIT_MAX_LEVELS),
                ("layers_per_block", C.c_int), ("cross_attention_dim", C.c_int),
                ("heads", C.c_int), ("norm_num_groups", C.c_int)]


class VaeCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("latent_channels", C.c_int), ("n_levels", C.c_int),
                ("block_out_channels", C.c_int * 4), ("layers_per_block", C.c_int),
                ("norm_num_groups", C.c_int)]


class DdpmCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_ch", C.c_int), ("ch", C.c_int), ("n_levels", C.c_int),
                ("ch_mult", C.c_int * 8), ("attn_level", C.c_int * 8), ("num_res_blocks", C.c_int),
                ("image_size", C.c_int)]


class VitCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "layers", "heads", "patch_size", "input_resolution")]


class TextCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "layers", "heads", "vocab_size", "context_length", "proj_dim")]


class ClipImgCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "layers", "heads", "patch_size", "input_resolution", "embed_dim")]


class DinoCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "layers", "heads", "patch_size", "input_resolution", "key_layer")]


class P2PPlan(C.Structure):
    _fields_ = [("mode", C.c_int), ("n_pairs", C.c_int),
                ("pair_src", C.c_void_p), ("pair_tar", C.c_void_p),
                ("singles", C.c_void_p), ("n_single", C.c_int),
                ("qk_src", C.c_void_p), ("mixT", C.c_void_p), ("bvec", C.c_void_p),
                ("h_store", C.POINTER(C.c_void_p)), ("n_store", C.c_int),
                ("kv_src", C.c_void_p), ("kv_first_block", C.c_int),
                ("qk_first_block", C.c_int), ("qk_max_tokens", C.c_int), ("feat_src", C.c_void_p), ("feat_resblock", C.c_int),
                ("h_store_self", C.POINTER(C.c_void_p)), ("n_store_self", C.c_int),
                ("masa_rows", C.c_void_p), ("h_masa_rows", C.POINTER(C.c_int32)), ("n_masa_rows", C.c_int),
                ("h_masa_cls_q", C.POINTER(C.c_void_p)), ("h_masa_cls_k", C.POINTER(C.c_void_p)),
                ("h_masa_tokens", C.POINTER(C.c_int32)), ("n_masa_res", C.c_int),
                ("masa_auto", C.c_int), ("masa_thres", C.c_float), ("masa_images", C.c_int),
                ("masa_ref_tokens", C.c_void_p), ("n_masa_ref", C.c_int), ("masa_cur_tokens", C.c_void_p), ("n_masa_cur", C.c_int),
                ("masa_ws", C.c_void_p), ("masa_ws_bytes", C.c_size_t),
                ("h_masa_dump", C.POINTER(C.c_void_p)), ("n_masa_dump", C.c_int)]


class StepCoef(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("sqrt_ab_t", "sqrt_1m_ab_t", "sqrt_ab_prev", "dir_coef",
                                         "noise_coef", "w_src", "w_hat", "w_tar", "coeff", "w_rec")]


def _family(name, cfg, finalizes, workspace_args):
    """The entries every network family has: hedit_<name>_create (with its cfg struct, if it has one) / destroy / num_params /
    param_name / param_shape / load / missing / workspace_bytes(handle, *workspace_args), and finalize where the family packs in a
    step of its own."""
    sigs = {"create": (C.c_int, ([C.POINTER(cfg)] if cfg else []) + [C.POINTER(C.c_void_p)]),
            "destroy": (None, [C.c_void_p]),
            "num_params": (C.c_int, [C.c_void_p]),
            "param_name": (C.c_char_p, [C.c_void_p, C.c_int]),
            "param_shape": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
            "load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p]),
            "missing": (C.c_int, [C.c_void_p]),
            "workspace_bytes": (C.c_size_t, [C.c_void_p] + workspace_args)}
    if finalizes:
        sigs["finalize"] = (C.c_int, [C.c_void_p, C.c_void_p])
    return {f"hedit_{name}_{k}": v for k, v in sigs.items()}


_SIGS = {    "hedit_last_error": (C.c_char_p, []),
    "hedit_version": (C.c_int, []),
    **_family("unet", UnetCfg, False, [C.c_int] * 3),
    "hedit_unet_param_bf16_exact": (C.c_int, [C.c_void_p, C.c_int]),
    "hedit_unet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                     C.c_int, C.POINTER(P2PPlan), C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "hedit_unet_forward_shared": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_float, C.c_void_p, C.c_int,
                                            C.c_int, C.c_int, C.POINTER(P2PPlan), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_unet_context_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "hedit_unet_context_destroy": (None, [C.c_void_p]),
    "hedit_unet_forward_bound": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                           C.c_int, C.POINTER(P2PPlan), C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p]),
    "hedit_unet_forward_shared_bound": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_float, C.c_void_p, C.c_int,
                                                  C.c_int, C.c_int, C.POINTER(P2PPlan), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_unet_create_grad": (C.c_int, [C.POINTER(UnetCfg), C.POINTER(C.c_void_p)]),
    "hedit_unet_grad_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "hedit_unet_forward_keep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_unet_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_unet_create_grad_ctx": (C.c_int, [C.POINTER(UnetCfg), C.POINTER(C.c_void_p)]),
    "hedit_unet_backward_ctx": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_unet_release": (None, [C.c_void_p]),
    "hedit_unet_vjp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_unet_set_attn_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_unet_num_store_layers": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hedit_unet_store_layer_info": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                              C.POINTER(C.c_int)]),
    "hedit_prof_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hedit_prof_reset": (C.c_int, [C.c_void_p]),
    "hedit_prof_collect": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int64)]),
    "hedit_prof_collect_bytes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "hedit_prof_records": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    "hedit_step_base": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_int, C.POINTER(StepCoef), C.c_void_p]),
    "hedit_step_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(StepCoef), C.c_void_p]),
    "hedit_step_invert": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.POINTER(StepCoef), C.c_void_p]),
    "hedit_step_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(StepCoef),
                                    C.c_void_p]),
    "hedit_step_tweedie": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "hedit_step_style": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "hedit_step_ef_seed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "hedit_step_ef_style": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "hedit_local_blend": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "hedit_local_blend_sub": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "hedit_attn_aggregate": (C.c_int, [C.POINTER(C.c_void_p)] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    **_family("ddpm", DdpmCfg, False, [C.c_int]),
    "hedit_ddpm_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "hedit_ddpm_create_grad": (C.c_int, [C.POINTER(DdpmCfg), C.POINTER(C.c_void_p)]),
    "hedit_ddpm_grad_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "hedit_ddpm_forward_keep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]),
    "hedit_ddpm_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_ddpm_release": (None, [C.c_void_p]),
    "hedit_ddpm_vjp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p]),
    **_family("irse50", None, True, [C.c_int]),
    "hedit_irse50_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_irse50_cos_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    **_family("lpips", None, True, [C.c_int] * 3),
    "hedit_lpips_feature_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "hedit_lpips_source": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "hedit_lpips_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    **_family("faceparse", None, True, [C.c_int] * 3),
    "hedit_faceparse_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]),
    "hedit_face_mask_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hedit_face_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    **_family("vit", VitCfg, True, [C.c_int]),
    "hedit_vit_gram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_vit_gram_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    **_family("text", TextCfg, True, [C.c_int] * 2),
    "hedit_text_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_size_t, C.c_void_p]),
    **_family("clipimg", ClipImgCfg, True, [C.c_int]),
    "hedit_clipimg_set_slices": (C.c_int, [C.c_void_p, C.c_int]),
    "hedit_clipimg_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    **_family("sqlpips", None, True, [C.c_int] * 3),
    "hedit_sqlpips_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]),
    **_family("dino", DinoCfg, True, [C.c_int] * 2),
    "hedit_dino_set_slices": (C.c_int, [C.c_void_p, C.c_int]),
    "hedit_dino_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_dino_structure_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p]),
    "hedit_pixel_metrics_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hedit_pixel_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "hedit_image_prep_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hedit_image_prep": (C.c_int, [C.c_void_p] + [C.c_int] * 9 + [C.c_void_p, C.c_void_p, C.c_int] * 2 + [C.c_int, C.c_int] +
                         [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "hedit_clip_direction": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    **_family("vae", VaeCfg, False, [C.c_int] * 4),
    "hedit_vae_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "hedit_vae_decode_vjp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_vae_decode_keep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]),
    "hedit_vae_decode_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_vae_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "hedit_axis_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int,
                                 C.c_void_p]),
    "hedit_k_gemm_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hedit_k_gemm_canonical_chunk": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "hedit_k_gemm_plan_splits": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hedit_k_gemm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 13 +
                     [C.c_void_p, C.c_void_p]),
    "hedit_k_conv_gn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 12 +
                        [C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_k_groupnorm_from_parts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "hedit_k_pack_geglu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_gemm_geglu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    "hedit_test_set_flags": (C.c_int, [C.c_int]),
    "hedit_storage_is_f16": (C.c_int, []),
    "hedit_k_lin_chain_stream_bytes": (C.c_size_t, [C.c_int]),
    "hedit_k_lin_chain_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "hedit_k_lin_chain": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_lin_chain_sched": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_groupnorm_affine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "hedit_k_ffn_channels": (C.c_int, []),
    "hedit_k_ffn_stream_bytes": (C.c_size_t, [C.c_int]),
    "hedit_k_ffn_bias_bytes": (C.c_size_t, []),
    "hedit_k_ffn_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_k_ffn_chain": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                    C.c_void_p]),
    "hedit_k_ffn_fused": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_groupnorm_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hedit_k_groupnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "hedit_k_layernorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                    C.c_float, C.c_void_p]),
    "hedit_k_geglu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "hedit_k_self_attn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_k_masked_self_attn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_k_masa_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "hedit_k_masa_auto_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "hedit_k_cross_attn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P2PPlan), C.c_void_p,
                                     C.c_void_p]),
    "hedit_k_attn_probs": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_attn_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_pack_conv3x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_f32_to_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "hedit_k_groupnorm_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hedit_k_groupnorm_bwd_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hedit_k_groupnorm_bwd": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "hedit_k_softmax_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p]),
    "hedit_k_softmax_blockdiag": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "hedit_k_softmax_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p]),
    "hedit_k_transpose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_sum2x2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_pack_conv3x3_dgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_pack_conv3x3_s2_dgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_conv3x3_s2_dgrad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p]),
    "hedit_k_slice_add": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "hedit_k_pack_linear_t": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_flip_oihw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_attn_bwd_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "hedit_k_attn_bwd": (C.c_int, [C.c_void_p, C.c_int] * 6 + [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p]),
    "hedit_k_cross_attn_bwd_q": (C.c_int, [C.c_void_p, C.c_int] * 6 + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_cross_attn_bwd_kv_ws_bytes": (C.c_size_t, [C.c_int] * 4),
    "hedit_k_cross_attn_bwd_kv": (C.c_int, [C.c_void_p, C.c_int] * 5 + [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "hedit_k_layernorm_bwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_float, C.c_void_p]),
    "hedit_k_groupnorm_bwd_any": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_void_p, C.c_void_p]),
    "hedit_k_geglu_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "hedit_k_conv3x3_s2_dgrad_pad1": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p]),
    # single kernels of the precise family (pnet.hip, encoder.hip, vit.hip's gradient kernels)
    "hedit_k_split3_geometry": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hedit_k_split3": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 8 +
                       [C.c_int64, C.c_void_p]),
    "hedit_k_pack_split3_w": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 9 + [C.c_void_p]),
    "hedit_k_precise_conv_ws_bytes": (C.c_size_t, [C.c_int] * 9),
    "hedit_k_precise_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] +
                             [C.c_int] * 10 + [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t, C.c_void_p]),
    "hedit_k_bn_affine": (C.c_int, [C.c_void_p] * 4 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_bn_fold_bias": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "hedit_k_act": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_se_nslab": (C.c_int, [C.c_int]),
    "hedit_k_se_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_se_fc": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_se_combine": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_se_bwd_reduce": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]),
    "hedit_k_se_fc_bwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_unit_bwd_combine": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_scale_cols": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_void_p]),
    "hedit_k_face_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "hedit_k_face_pool_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "hedit_k_cos_head": (C.c_int, [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "hedit_k_lpips_prep": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
    "hedit_k_lpips_prep_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_maxpool2": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_maxpool2_bwd": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_lpips_head": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_float, C.c_void_p]),
    "hedit_k_lpips_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "hedit_k_enc_patchify": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_enc_tokens": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p]),
    "hedit_k_enc_gather_rows": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "hedit_k_enc_ln": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_float, C.c_void_p]),
    "hedit_k_enc_add_bias_res": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_void_p]),
    "hedit_k_vit_ln_bwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_void_p]),
    "hedit_k_vit_attn_fwd": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_vit_attn_bwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p]),
    "hedit_k_vit_drop_cls": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]),
    "hedit_k_vit_gram_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
}

EXPORTS = tuple(_SIGS.keys())


class HipLibraryMissing(RuntimeError):
    pass


_lib = None


def lib():
    """The loaded library (loads on first use).  There is deliberately no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build it with `python h-edit_amd/build.py{' --f16' if STORAGE == 'f16' else ''}` "
                "(hipcc --offload-arch=gfx950); hedit has no CPU/eager fallback")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)     # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if bool(l.hedit_storage_is_f16()) != (STORAGE == "f16"):
            raise HipLibraryMissing(f"{LIB_PATH} was not built for HEDIT_STORAGE={STORAGE}")
        _lib = l
    return _lib


def storage_dtype():
    """torch dtype of the 16-bit tensors the kernel-level entries (hedit_k_*) and the P2P mix tables exchange with the library"""
    import torch
    return torch.float16 if STORAGE == "f16" else torch.bfloat16


class HipError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise HipError(f"libhedit_hip error {rc}: {lib().hedit_last_error().decode()}")


def ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def cur_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
