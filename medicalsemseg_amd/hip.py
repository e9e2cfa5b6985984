"""ctypes binding of ``libmsseg_hip.so`` (C ABI: ``include/msseg.h``) + thin tensor-level wrappers.

There is NO CPU fallback: if the shared library is missing, or a tensor is not on a GPU, these
functions raise.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSSEG_LIB") or os.path.join(_HERE, "libmsseg_hip.so")   # MSSEG_LIB: A/B another build

F32, BF16 = 0, 1
_DT = {torch.float32: F32, torch.bfloat16: BF16}
_LAB = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2, torch.int64: 3}

_lib = None

_vp, _ll, _i, _f, _sz = C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_size_t

# name -> argtypes (every symbol include/msseg.h declares; tests check the .so exports all of them)
SIGNATURES = {
    "msseg_abi_version": ([], _i),
    "msseg_last_error": ([], C.c_char_p),
    "msseg_num_cus": ([], _i),
    "msseg_packed_weight_bytes": ([_i, _i, _i, _i, _i], _sz),
    "msseg_pack_weights": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _ll, _ll, _ll, _ll, _ll, _i, _i, _vp], _i),
    "msseg_pack_weights_batch": ([_vp, _i, _ll, _ll, _i, _vp], _i),
    "msseg_cout_block": ([_i], _i),
    "msseg_conv3d_k3_cout_block": ([_i, _i, _i, _i, _i], _i),
    "msseg_conv3d_k3_variant": ([_i, _i, _i, _i, _i], _i),
    "msseg_conv3d_k3_kernel": ([_i, _i, _i, _i, _i, _i, _i], _i),
    "msseg_conv3d_k3_resident_per_cu": ([_i, _i, _i, _i, _i, _i, _i], _i),
    "msseg_conv3d_k3_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_k3_fwd_accumulate": ([_vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_k3_fwd_split": ([_vp, _ll, _vp, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp], _i),
    "msseg_conv3d_k3_split_ok": ([_i, _i, _i, _i, _i, _i, _i, _i], _i),
    "msseg_dwconv3d_k3_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_dwconv3d_k3_wgrad": ([_vp, _ll, _vp, _ll, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_dwconv3d_fwd": ([_vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_dwconv3d_wgrad_workspace_bytes": ([_i, _i, _i, _i, _i, _i, _i], _sz),
    "msseg_dwconv3d_wgrad": ([_vp, _ll, _vp, _ll, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_focal_spatial_sum": ([_vp, _ll, _vp, _ll, _vp, _vp, _vp, _f, _i, _i, _ll, _i, _vp, _sz, _i, _vp], _i),
    "msseg_focal_aggregate_fwd": ([_vp, _vp, _vp, _ll, _vp, _vp, _i, _ll, _i, _i, _vp], _i),
    "msseg_focal_aggregate_bwd": ([_vp, _vp, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp, _ll, _i, _i, _ll, _i, _i, _vp], _i),
    "msseg_focal_mul_fwd": ([_vp, _ll, _vp, _vp, _ll, _i, _i, _vp], _i),
    "msseg_focal_mul_bwd": ([_vp, _vp, _ll, _vp, _vp, _ll, _vp, _ll, _i, _i, _vp], _i),
    "msseg_interp_trilinear_fwd": ([_vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_interp_trilinear_bwd_workspace_bytes": ([_i, _i, _i, _i, _i, _i, _i, _i], _sz),
    "msseg_interp_trilinear_bwd": ([_vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_kv_attention_fwd": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _vp], _i),
    "msseg_kv_attention_bwd_workspace_bytes": ([_i, _i, _i, _i, _i], _sz),
    "msseg_kv_attention_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _sz, _i, _vp], _i),
    "msseg_scale_channels": ([_vp, _vp, _vp, _i, _ll, _i, _i, _vp], _i),
    "msseg_reduce_scratch_bytes": ([], _sz),
    "msseg_conv3d_k3_dgrad_inbwd": ([_vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp, _ll, _vp, _ll, _vp, _f, _f, _vp,
                                     _vp, _vp, _i, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_k1_dgrad_inbwd": ([_vp, _ll, _vp, _vp, _ll, _i, _ll, _i, _i, _vp, _ll, _vp, _ll, _vp, _f, _f, _vp,
                                     _vp, _vp, _i, _vp, _sz, _i, _vp], _i),
    "msseg_deconv_k2s2_bwd_fused": ([_vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp, _ll, _vp, _ll, _vp, _f, _f,
                                     _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_k3s2_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_zero_stuff2": ([_vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_window_attention_fwd": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _ll, _i, _vp], _i),
    "msseg_window_attention_bwd": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _ll, _i,
                                    _vp, _sz, _vp], _i),
    "msseg_window_attention_bwd_workspace_bytes": ([_i, _i, _i, _i, _i, _i, _i, _i, _i, _ll, _i], _sz),
    "msseg_rel_bias_affine_fold": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "msseg_rel_bias_affine_grad_workspace_bytes": ([_i, _i], _sz),
    "msseg_rel_bias_affine_grad": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp], _i),
    "msseg_layernorm_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _vp, _vp, _ll, _i, _f, _i, _vp], _i),
    "msseg_layernorm_bwd": ([_vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _ll, _i, _i, _vp], _i),
    "msseg_layernorm_bwd_add": ([_vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _vp, _ll, _ll, _i, _i, _vp], _i),
    "msseg_layernorm_param_grad": ([_vp, _ll, _vp, _vp, _vp, _ll, _vp, _vp, _i, _ll, _i, _vp, _sz, _i, _vp], _i),
    "msseg_gelu_fwd": ([_vp, _vp, _ll, _i, _vp], _i),
    "msseg_gelu_bwd": ([_vp, _vp, _vp, _ll, _i, _vp], _i),
    "msseg_linear_wgrad_ok": ([_ll, _i, _i, _i], _i),
    "msseg_linear_wgrad": ([_vp, _ll, _vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_linear_gelu_ok": ([_ll, _i, _i, _i], _i),
    "msseg_linear_gelu_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _vp, _ll, _ll, _i, _i, _i, _vp], _i),
    "msseg_linear_gelu_bwd": ([_vp, _ll, _vp, _vp, _ll, _vp, _ll, _ll, _i, _i, _i, _vp], _i),
    "msseg_linear_add_ok": ([_ll, _i, _i, _i], _i),
    "msseg_linear_add_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _vp, _ll, _ll, _i, _i, _i, _vp], _i),
    "msseg_conv3d_stem_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_stem_norm_fwd": ([_vp, _ll, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_conv3d_k1_head_norm_fwd": ([_vp, _ll, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _ll, _i, _ll, _i, _i, _i, _vp], _i),
    "msseg_conv3d_k1_head_bwd_fused": ([_vp, _ll, _vp, _vp, _ll, _i, _ll, _i, _i, _vp, _ll, _vp, _vp, _vp, _f, _f, _vp, _vp,
                                        _vp, _i, _vp, _i, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_k1_head_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _ll, _i, _i, _i, _vp], _i),
    "msseg_conv3d_k1_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _ll, _i, _i, _i, _vp], _i),
    "msseg_conv3d_gather_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_deconv_k2s2_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_deconv_k2s2_bwd_data": ([_vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_deconv_k4s4_fwd": ([_vp, _ll, _vp, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_deconv_k4s4_bwd_data": ([_vp, _ll, _vp, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_wgrad_workspace_bytes": ([_i, _i, _i], _sz),
    "msseg_conv3d_k3_wgrad_kernel": ([_i, _i, _i, _i, _i, _i, _i], _i),
    "msseg_conv3d_k3_wgrad": ([_vp, _ll, _vp, _ll, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_k1_wgrad": ([_vp, _ll, _vp, _ll, _vp, _ll, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_stem_wgrad_inbwd": ([_vp, _ll, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _vp, _f, _f, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_conv3d_gather_wgrad": ([_vp, _ll, _vp, _ll, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_deconv_k2s2_wgrad": ([_vp, _ll, _vp, _ll, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_deconv_k4s4_wgrad": ([_vp, _ll, _vp, _ll, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_channel_stats": ([_vp, _ll, _vp, _i, _ll, _i, _vp, _sz, _i, _vp], _i),
    "msseg_instnorm_act_fwd": ([_vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _i, _ll, _i, _f, _f, _i, _vp], _i),
    "msseg_instnorm_act_poolbwd_reduce": ([_vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _i,
                                           _i, _i, _i, _i, _i, _f, _f, _vp, _sz, _i, _vp], _i),
    "msseg_instnorm_act_pool_fwd": ([_vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _f, _f, _i, _vp], _i),
    "msseg_instnorm_act_bwd_reduce": ([_vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _i, _i, _ll, _i, _f, _f, _vp, _sz, _i, _vp], _i),
    "msseg_instnorm_act_bwd_apply_head": ([_vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _i, _vp, _vp, _ll, _i, _ll, _i, _f, _f, _i, _vp], _i),
    "msseg_instnorm_act_bwd_apply": ([_vp, _ll, _vp, _vp, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _ll, _vp, _ll, _i, _ll, _i, _f, _f, _i, _vp], _i),
    "msseg_maxpool2_fwd": ([_vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_maxpool2_bwd": ([_vp, _ll, _vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_ncdhw_to_ndhwc": ([_vp, _i, _vp, _ll, _i, _i, _i, _ll, _vp], _i),
    "msseg_ndhwc_to_ncdhw": ([_vp, _ll, _i, _vp, _i, _i, _i, _ll, _vp], _i),
    "msseg_channel_sum": ([_vp, _ll, _vp, _ll, _i, _i, _vp, _sz, _i, _vp], _i),
    "msseg_axpy_rows": ([_vp, _vp, _vp, _vp, _i, _ll, _i, _vp], _i),
    "msseg_add": ([_vp, _ll, _vp, _ll, _vp, _ll, _ll, _i, _i, _vp], _i),
    "msseg_seg_loss_partials": ([_vp, _ll, _i, _vp, _i, _vp, _vp, _i, _ll, _i, _i, _vp], _i),
    "msseg_seg_loss_fwd": ([_vp, _ll, _i, _vp, _i, _vp, _vp, _vp, _i, _ll, _i, _f, _f, _i, _f, _f, _vp, _sz, _vp], _i),
    "msseg_seg_loss_finalize": ([_vp, _vp, _i, _ll, _i, _f, _f, _i, _f, _f, _vp], _i),
    "msseg_seg_loss_bwd": ([_vp, _ll, _i, _vp, _i, _vp, _vp, _vp, _ll, _i, _ll, _i, _f, _f, _i, _f, _f, _vp], _i),
    "msseg_adamw_step": ([_vp, _vp, _vp, _vp, _vp, _ll, _f, _f, _f, _f, _f, _i, _vp, _vp, _vp], _i),
    "msseg_sumsq": ([_vp, _ll, _vp, _vp, _i, _vp], _i),
    "msseg_sw_normalize": ([_vp, _vp, _i, _ll, _vp], _i),
    "msseg_box_copy": ([_vp, _ll, _i, _i, _i, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_merge_gather_fwd": ([_vp, _ll, _i, _i, _i, _vp, _ll, _i, _i, C.c_uint, _i, _vp], _i),
    "msseg_merge_gather_bwd": ([_vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, C.c_uint, _i, _vp], _i),
    "msseg_region_loss_partials": ([_vp, _ll, _i, _vp, _i, _vp, _vp, _i, _ll, _i, _i, _vp, _vp], _i),
    "msseg_region_loss_fwd": ([_vp, _ll, _i, _vp, _i, _vp, _vp, _vp, _i, _ll, _i, _f, _f, _i, _f, _f, _vp, _vp, _sz, _vp], _i),
    "msseg_region_loss_finalize": ([_vp, _vp, _i, _ll, _i, _f, _f, _i, _f, _f, _vp], _i),
    "msseg_region_loss_bwd": ([_vp, _ll, _i, _vp, _i, _vp, _vp, _vp, _ll, _i, _ll, _i, _f, _f, _i, _f, _f, _vp, _vp], _i),
    "msseg_region_decode_u8": ([_vp, _i, _ll, _vp, _vp, _vp, _vp], _i),
    "msseg_region_counts_u8": ([_vp, _vp, _ll, _i, _vp, _vp, _vp, _sz, _vp], _i),
    "msseg_argmax_u8": ([_vp, _i, _ll, _vp, _vp], _i),
    "msseg_resample_nearest_u8": ([_vp, _i, _i, _i, _vp, _i, _i, _i, _vp], _i),
    "msseg_majority_vote_u8": ([_vp, _i, _ll, _i, _vp, _vp], _i),
    "msseg_aug_crop_batch": ([_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp], _i),
    "msseg_intensity_prep": ([_vp, _i, _i, _i, _i, _i, _i, _f, _f, _i, _f, _f, _vp, _vp, _vp], _i),
    "msseg_resample_spacing": ([_vp, _i, _i, _i, _i, _i, _vp, _i, _i, _i, C.c_double, C.c_double, C.c_double, _vp], _i),
    "msseg_crop_pad_copy": ([_vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _f, _i, _vp], _i),
    "msseg_slab_counts": ([_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp], _i),
    "msseg_pick_voxels": ([_vp, _i, _vp, _i, _i, _f, _i, _vp, _vp], _i),
    "msseg_class_candidate_mask": ([_vp, _vp, _i, _i, _i, _f, _i, C.c_uint, _i, _vp, _vp, _vp], _i),
    "msseg_class_slab_counts": ([_vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp], _i),
    "msseg_class_pick_voxels": ([_vp, _vp, _i, _vp, _i, _i, _f, _i, _vp, _vp], _i),
    "msseg_volume_stats_scratch_bytes": ([_i], _sz),
    "msseg_select_f32": ([_vp, _i, _ll, _vp, _i, _vp, _i, _vp, _sz, _vp, _vp], _i),
    "msseg_masked_moments": ([_vp, _i, _ll, _vp, _ll, _vp, _sz, _vp, _vp], _i),
    "msseg_zscore_apply": ([_vp, _i, _ll, _vp, _vp], _i),
    "msseg_aug_crop_multi": ([_vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp], _i),
    "msseg_aug_crop_affine": ([_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i, _f, _vp], _i),
    "msseg_intensity_aug_workspace_bytes": ([_i, _i, _i, _i, _i], _sz),
    "msseg_intensity_aug": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _sz, _vp], _i),
    "msseg_intensity_noise_bits": ([C.c_uint, C.c_uint, _ll, _ll, _vp, _vp], _i),
    "msseg_sw_gather_batch": ([_vp, _ll, _vp, _ll, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp], _i),
    "msseg_sw_blend_batch": ([_vp, _ll, _i, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_deconv_k2s2_bwd_partials_ok": ([_i, _i, _i], _i),
    "msseg_deconv_k2s2_bwd_partials": ([_vp, _ll, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_conv3d_k3_small_ok": ([_i, _i, _i, _i, _i, _i, _i], _i),
    "msseg_conv3d_k3_small_workspace_bytes": ([_i, _i, _i, _i, _i, _i], _sz),
    "msseg_conv3d_k3_small_stage_groups": ([_i, _i, _i, _i, _i, _i], _i),
    "msseg_conv3d_k3_small_partials": ([_vp, _ll, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_conv3d_k3_small_fwd_finish": ([_vp, _i, _vp, _vp, _vp, _f, _f, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _i, _i,
                                          _i, _i, _i, _vp], _i),
    "msseg_conv3d_k3_small_bwd_finish": ([_vp, _i, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _f, _f, _vp, _vp, _i, _i, _i, _i, _i,
                                          _i, _vp], _i),
    "msseg_avgpool3d_k3": ([_vp, _ll, _vp, _ll, _i, _i, _i, _i, _i, _i, _vp], _i),
    "msseg_hd_edges": ([_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "msseg_hd_directed_workspace_bytes": ([_i, _i, _i], _sz),
    "msseg_hd_directed_hist": ([_vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _i, _vp], _i),
    "msseg_sd_directed_workspace_bytes": ([_i, _i, _i], _sz),
    "msseg_sd_directed_mm": ([_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp], _i),
    "msseg_sd_summary_scratch_bytes": ([], _sz),
    "msseg_sd_summary": ([_vp, _ll, _vp, _i, _vp, _i, _vp, _sz, _vp, _vp], _i),
    "msseg_keep_largest_u8": ([_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "msseg_postprocess_u8": ([_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _i),
    "msseg_restore_native_u8": ([_vp, _i, _i, _vp, _vp, _vp], _i),
    "msseg_ktimer_enable": ([_i], _i),
    "msseg_ktimer_reset": ([], _i),
    "msseg_ktimer_count": ([], _i),
    "msseg_ktimer_get": ([_i, C.c_char_p, _i, C.POINTER(C.c_float)], _i),
}


def load_library(path: Optional[str] = None):
    """dlopen the HIP library and set argtypes.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(or `make -C medicalsemseg_amd/csrc`).  There is no CPU fallback.")
    lib = C.CDLL(p)
    for name, (args, res) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    if lib.msseg_abi_version() != 3:
        raise RuntimeError("libmsseg_hip.so ABI version mismatch")
    _lib = lib
    return lib


def lib():
    real = _lib if _lib is not None else load_library()
    if TIMER.enabled:
        return _TimedLib(real)
    return real


class MssegError(RuntimeError):
    pass


def _ck(rc: int, what: str):
    if rc != 0:
        raise MssegError(f"{what} failed ({rc}): {lib().msseg_last_error().decode()}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("medicalsemseg_amd kernels run on the GPU only (got a CPU tensor); "
                               "there is no CPU fallback")


def dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype} (float32 / bfloat16 only)")


def ld(t: torch.Tensor) -> int:
    """voxel stride of a channels-last [..., C] tensor (possibly a channel slice of a wider buffer)."""
    C = t.shape[-1]
    if C > 1 and t.stride(-1) != 1:
        raise ValueError("channels-last tensor must have unit channel stride")
    # voxel stride = stride of the innermost spatial dim that has extent > 1 (size-1 dims carry arbitrary strides)
    l = None
    exp = None
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] > 1:
            if l is None:
                l = t.stride(d)
                exp = l * t.shape[d]
            else:
                if t.stride(d) != exp:
                    raise ValueError(f"tensor is not a dense channels-last volume: shape {tuple(t.shape)} "
                                     f"stride {t.stride()}")
                exp *= t.shape[d]
    if l is None:
        l = C
    if l < C:
        raise ValueError("voxel stride smaller than the channel count")
    return l


def _nbytes(*ts) -> float:
    """algorithmic bytes of a streaming pass: every operand read or written once"""
    return float(sum(t.numel() * t.element_size() for t in ts if t is not None))


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------------------------
# weights
# --------------------------------------------------------------------------------------------
def cout_block(M: int) -> int:
    return lib().msseg_cout_block(M)


def conv_k3_cout_block(N, D, H, W, cout) -> int:
    return lib().msseg_conv3d_k3_cout_block(N, D, H, W, cout)


def conv_k3_resident_per_cu(N, D, H, W, cin, cout, dtype) -> int:
    """workgroups of the generic conv k3 kernel planned for this problem that one CU holds at the LDS size of a batch of N"""
    r = lib().msseg_conv3d_k3_resident_per_cu(N, D, H, W, cin, cout, _DT[dtype])
    if r < 0:
        _ck(r, "conv3d_k3_resident_per_cu")
    return r


class PackJob(C.Structure):
    """mirror of msseg_pack_job (include/msseg.h)"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p),
                ("s_m1", C.c_longlong), ("s_m0", C.c_longlong), ("s_t", C.c_longlong), ("s_k1", C.c_longlong),
                ("s_k0", C.c_longlong), ("total", C.c_longlong),
                ("M", C.c_int), ("M0", C.c_int), ("T", C.c_int), ("K", C.c_int), ("K0", C.c_int), ("flip", C.c_int),
                ("cout_block", C.c_int), ("nkb", C.c_int)]


# the most recent pack_weights call as a (src, dst, PackJob) triple: layers.PackedCache registers it for the
# once-per-step batched refresh
LAST_PACK_JOBS = []     # (src, dst, PackJob) of every image packed since a PackedCache last cleared the list


def pack_weights(src: torch.Tensor, dtype: torch.dtype, M, M0, T, K, K0, s_m1, s_m0, s_t, s_k1, s_k0, flip=False,
                 out: Optional[torch.Tensor] = None, cb: Optional[int] = None) -> torch.Tensor:
    _need_gpu(src)
    assert src.dtype == torch.float32      # any layout the explicit strides describe (a channel slice of a conv weight)
    cb = cb or cout_block(M)
    nbytes = lib().msseg_packed_weight_bytes(M, T, K, cb, _DT[dtype])
    esz = 4 if dtype == torch.float32 else 2
    if out is None:
        out = torch.empty(nbytes // esz, dtype=dtype, device=src.device)
    assert out.numel() * esz == nbytes
    _ck(lib().msseg_pack_weights(_p(src), _p(out), _DT[dtype], M, M0, T, K, K0, s_m1, s_m0, s_t, s_k1, s_k0,
                                 int(flip), cb, _stream()), "pack_weights")
    LAST_PACK_JOBS.append((src, out, PackJob(_p(src), _p(out), s_m1, s_m0, s_t, s_k1, s_k0, nbytes // esz, M, M0, T, K, K0,
                                             int(flip), cb, -(-K // (64 // esz)))))
    return out


def pack_weights_batch(table: torch.Tensor, njobs: int, max_total: int, sum_total: int, dtype: torch.dtype):
    """table: uint8 device tensor holding njobs consecutive PackJob structs; max_total / sum_total: largest / summed job.total"""
    _ck(lib().msseg_pack_weights_batch(_p(table), njobs, max_total, sum_total, _DT[dtype], _stream()), "pack_weights_batch")


def pack_conv_k3(w: torch.Tensor, dtype, dgrad=False, out=None, vol=None, cb=None):
    """w: [Cout, Cin, 3,3,3] fp32 (dense, or an input-channel slice w_full[:, a:b] of a dense weight: forward image only).
    Forward image W[co][tap][ci]; dgrad image W'[ci][26-tap][co].
    vol = (N, D, H, W) of the stride-1 problem the image will be used for (selects the cout block), or cb = the block."""
    co, ci = w.shape[0], w.shape[1]
    if cb is None and vol is not None and out is None and dtype == torch.bfloat16 and (co if dgrad else ci) == 48 \
            and lib().msseg_conv3d_k3_kernel(*vol, 48, ci if dgrad else co, BF16) == 4:
        return pack_conv_k3_c48(w, dgrad)
    if not dgrad:
        cb = cb or (conv_k3_cout_block(*vol, co) if vol is not None else None)
        assert w.stride(1) == 27 and w.stride(4) == 1 and w.stride(0) % 27 == 0
        return pack_weights(w, dtype, co, co, 27, ci, ci, 0, w.stride(0), 1, 0, 27, False, out, cb)
    assert w.is_contiguous()
    cb = cb or (conv_k3_cout_block(*vol, ci) if vol is not None else None)
    return pack_weights(w, dtype, ci, ci, 27, co, co, 0, 27, 1, 0, ci * 27, True, out, cb)


def pack_conv_k3_c48(w: torch.Tensor, dgrad=False):
    """bf16 image of the 48-input-channel ping-pong kernel (csrc/conv3d_k3_c48.hip; msseg_conv3d_k3_kernel() == 4) for the
    layer y = conv(x[48 ch], w) -- w: [Cout, 48, 3,3,3] (dense, or an input-channel slice of a dense weight) -- or, dgrad,
    for dx = conv(dy[48 ch], w') of a layer w: [48, Cin, 3,3,3].  Four msseg_pack_weights images back to back, 16-wide cout
    blocks: channels 0..31 of the 27 taps; channels 32..47 of the tap pairs (kw 0, kw 1) per (kd, kh); of (kd 0, kd 1)
    at kw 2 per kh; of (kd 2, kw 2) per kh (upper half of the k-step zero)."""
    co, ci = w.shape[0], w.shape[1]
    n_el = w.untyped_storage().nbytes() // 4 - w.storage_offset()
    flat = w.as_strided((n_el,), (1,))                            # the storage from w's first element on
    if not dgrad:
        assert ci == 48 and w.stride(1) == 27 and w.stride(4) == 1 and w.stride(0) % 27 == 0
        M, s_m, s_c = co, w.stride(0), 27                         # strides of the output / input channel index
    else:
        assert co == 48 and w.is_contiguous()
        M, s_m, s_c = ci, 27, ci * 27
    assert M % 16 == 0
    ncb = M // 16
    buf = torch.empty(ncb * 42 * 512, dtype=torch.bfloat16, device=w.device)
    o = [0, ncb * 27 * 512, ncb * 36 * 512, ncb * 39 * 512, ncb * 42 * 512]
    rest = 32 * s_c
    bf = torch.bfloat16
    pack_weights(flat, bf, M, M, 27, 32, 32, 0, s_m, 1, 0, s_c, dgrad, buf[o[0]:o[1]], 16)
    if not dgrad:
        # T index = kd * 3 + kh (x 3 taps); k = [16 channels of tap A | 16 channels of tap B]
        pack_weights(flat[rest:], bf, M, M, 9, 32, 16, 0, s_m, 3, 1, s_c, False, buf[o[1]:o[2]], 16)       # B = kw + 1
        pack_weights(flat[rest + 2:], bf, M, M, 3, 32, 16, 0, s_m, 3, 9, s_c, False, buf[o[2]:o[3]], 16)   # kw 2: B = kd + 1
        pack_weights(flat[rest + 20:], bf, M, M, 3, 16, 16, 0, s_m, 3, 0, s_c, False, buf[o[3]:o[4]], 16)  # (kd 2, kw 2)
    else:
        # the image's tap (kd, kh, kw) is the layer's tap (2-kd, 2-kh, 2-kw): the packer's flip reverses the T index, the
        # base offset is the flipped kw / kd of tap A and tap B lies one tap / one plane BEFORE it
        pack_weights(flat[rest + 2:], bf, M, M, 9, 32, 16, 0, s_m, 3, -1, s_c, True, buf[o[1]:o[2]], 16)
        pack_weights(flat[rest + 18:], bf, M, M, 3, 32, 16, 0, s_m, 3, -9, s_c, True, buf[o[2]:o[3]], 16)
        pack_weights(flat[rest:], bf, M, M, 3, 16, 16, 0, s_m, 3, 0, s_c, True, buf[o[3]:o[4]], 16)
    return buf


def pack_conv_k1(w: torch.Tensor, dtype, dgrad=False, out=None):
    co, ci = w.shape[0], w.shape[1]
    if not dgrad:
        return pack_weights(w, dtype, co, co, 1, ci, ci, 0, ci, 0, 0, 1, False, out)
    return pack_weights(w, dtype, ci, ci, 1, co, co, 0, 1, 0, 0, ci, False, out)


def pack_conv_gather(w: torch.Tensor, dtype, out=None):
    """w: [Cout, Cin, k,k,k]; logical K index = tap*Cin + ci."""
    co, ci = w.shape[0], w.shape[1]
    kt = w.shape[2] * w.shape[3] * w.shape[4]
    return pack_weights(w, dtype, co, co, 1, ci * kt, ci, 0, ci * kt, 0, 1, kt, False, out)


def pack_deconv(w: torch.Tensor, dtype, bwd=False, out=None):
    """w: ConvTranspose3d weight [Cin, Cout, k,k,k], k = 2 or 4 (kernel = stride).  fwd: M = abc*Cout+co, K = ci.
    bwd-data: M = ci, K = abc*Cout+co.  abc = the child's index in the weight's own (a, b, c) order, k^3 children."""
    ci, co = w.shape[0], w.shape[1]
    nc = w.shape[2] * w.shape[3] * w.shape[4]
    if nc not in (8, 64) or not (w.shape[2] == w.shape[3] == w.shape[4]):
        raise NotImplementedError(f"transposed conv with kernel {tuple(w.shape[2:])}: only k = s = 2 and k = s = 4 are implemented")
    if not bwd:
        return pack_weights(w, dtype, nc * co, co, 1, ci, ci, 1, nc, 0, 0, co * nc, False, out)
    return pack_weights(w, dtype, ci, ci, 1, nc * co, co, 0, co * nc, 0, 1, nc, False, out)


# --------------------------------------------------------------------------------------------
# optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg)
# --------------------------------------------------------------------------------------------
class KernelTimer:
    """Per-launch timing with HIP events on the launch stream (bench.py's roofline leg).  While `enabled`, EVERY call into
    the library that launches kernels is bracketed by an event pair and filed under its entry point's name (`lib()` hands
    out a timing proxy), so the dominant group of a step is found by measurement; `launch()` lets a wrapper file a call
    under its own key with the call's algorithmic flops / bytes.  An entry point's time includes the small follow-up
    kernels it launches itself (statistics finalize, slab reduction); the main kernels' own durations come from the
    library's `msseg_ktimer_*` events, recorded directly around those launches (`ktimer_summary`)."""

    def __init__(self):
        self.records = {}
        self.enabled = False
        self._pending = None

    def launch(self, key, flops, nbytes, fn):
        if not self.enabled:
            return fn()
        self._pending = (key, flops, nbytes)
        try:
            return fn()
        finally:
            self._pending = None

    def call(self, name, cfn, args):
        ann, self._pending = self._pending, None
        key, flops, nbytes = ann if ann is not None else (name[6:], 0.0, 0.0)
        st = torch.cuda.current_stream()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        r = cfn(*args)
        e1.record(st)
        self.records.setdefault(key, []).append((e0, e1, flops, nbytes))
        return r

    def summary(self):
        out = {}
        for k, recs in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _, _ in recs]
            out[k] = {"launches": len(recs), "total_ms": sum(ms), "avg_ms": sum(ms) / len(ms),
                      "flops": sum(r[2] for r in recs), "bytes": sum(r[3] for r in recs)}
        return out


class _TimedLib:
    """what `lib()` returns while TIMER.enabled: every launching entry point goes through TIMER.call"""
    _QUERY = ("_bytes", "_block", "_variant", "_kernel", "_ok", "_groups", "abi_version", "last_error", "num_cus")

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.endswith(self._QUERY) or name.startswith("msseg_ktimer"):
            return fn
        return lambda *a: TIMER.call(name, fn, a)


def ktimer_enable(on: bool):
    """library-side event pairs directly around the main conv kernels (msseg_ktimer_*, include/msseg.h)"""
    load_library().msseg_ktimer_enable(int(on))


def ktimer_summary(reset=True):
    """{kernel name: {"launches", "total_ms", "avg_ms"}} of the launches recorded since the last reset (synchronises)"""
    L = load_library()
    torch.cuda.synchronize()
    out = {}
    buf = C.create_string_buffer(96)
    ms = C.c_float()
    for i in range(L.msseg_ktimer_count()):
        if L.msseg_ktimer_get(i, buf, 96, C.byref(ms)) == 0:
            r = out.setdefault(buf.value.decode(), {"launches": 0, "total_ms": 0.0})
            r["launches"] += 1
            r["total_ms"] += float(ms.value)
    for r in out.values():
        r["avg_ms"] = r["total_ms"] / r["launches"]
    if reset:
        L.msseg_ktimer_reset()
    return out


TIMER = KernelTimer()


# --------------------------------------------------------------------------------------------
# igemm forward-shaped ops.  x, y: [N, D, H, W, C] channels-last (views allowed)
# --------------------------------------------------------------------------------------------
_scratch_cache = {}


def scratch(device) -> torch.Tensor:
    """scratch for the deterministic two-launch reductions (one per device, stable address): blocks store partial rows past
    a reserved 256-byte header that no kernel reads or writes, and a second launch on the same stream adds them in a fixed
    order.  The C contract asks for no initialisation; the buffer is allocated as zeros all the same."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    buf = _scratch_cache.get(key)
    if buf is None:
        buf = torch.zeros(lib().msseg_reduce_scratch_bytes() + 256, dtype=torch.uint8, device=device)
        off = (-buf.data_ptr()) % 256
        buf = buf[off:off + lib().msseg_reduce_scratch_bytes()]
        _scratch_cache[key] = buf
    return buf


def conv3d_k3(x, wp, bias, y, cin, cout, stats=None):
    """stats: optional [N, cout, 2] fp32 output = (sum, sum of squares) of y (fused InstanceNorm statistics)."""
    _need_gpu(x, wp, y)
    N, D, H, W = x.shape[:4]
    nv = N * D * H * W
    esz = x.element_size()
    sc = scratch(x.device) if stats is not None else None

    def go():
        _ck(lib().msseg_conv3d_k3_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(y), ld(y), N, D, H, W, cin, cout, _p(stats),
                                      _p(sc), sc.numel() if sc is not None else 0, dt(x), _stream()), "conv3d_k3_fwd")
    key = "conv3d_k3_fwd"
    if TIMER.enabled:
        key += "/v%d" % lib().msseg_conv3d_k3_kernel(N, D, H, W, cin, cout, dt(x))
    TIMER.launch(key, 2.0 * nv * 27 * cin * cout, nv * (cin + cout) * esz + 27 * cin * cout * esz, go)
    return y


def conv3d_k3_split_ok(vol, cin, cout, split, dtype) -> bool:
    """does conv3d_k3_split take conv k3 cin -> cout on the grid vol = (N, D, H, W) with the output split at channel `split`?"""
    return dtype in _DT and bool(lib().msseg_conv3d_k3_split_ok(*vol, cin, cout, split, _DT[dtype]))


def conv3d_k3_split(x, wp, bias, ya, yb, cin, cout, stats=None, accumulate=False):
    """conv3d_k3 with the output channels [0, ca) written to ya and [ca, cout) to yb (ca = ya.shape[-1]): the same values as
    conv3d_k3 into one cout-wide tensor, as two tensors.  Ping-pong kernel only (conv3d_k3_split_ok); stats / accumulate are
    refused by the library."""
    _need_gpu(x, wp, ya, yb)
    N, D, H, W = x.shape[:4]
    nv = N * D * H * W
    esz = x.element_size()
    ca = ya.shape[-1]
    if tuple(ya.shape[:4]) != (N, D, H, W) or tuple(yb.shape[:4]) != (N, D, H, W) or ca + yb.shape[-1] != cout:
        raise ValueError("conv3d_k3_split: ya / yb must be [N, D, H, W, ca] and [N, D, H, W, cout - ca] on x's grid")

    def go():
        _ck(lib().msseg_conv3d_k3_fwd_split(_p(x), ld(x), _p(wp), _p(bias), _p(ya), ld(ya), _p(yb), ld(yb), ca, N, D, H, W,
                                            cin, cout, _p(stats), int(accumulate), dt(x), _stream()), "conv3d_k3_fwd_split")
    TIMER.launch("conv3d_k3_fwd/v3", 2.0 * nv * 27 * cin * cout, nv * (cin + cout) * esz + 27 * cin * cout * esz, go)
    return ya, yb


def conv3d_k3_accumulate(x, wp, y, cin, cout, stats):
    """y += conv k3 (x, packed image) on the ping-pong kernel; stats [N, cout, 2] = statistics of the sums"""
    _need_gpu(x, wp, y, stats)
    N, D, H, W = x.shape[:4]
    nv = N * D * H * W
    sc = scratch(x.device)
    TIMER.launch("conv3d_k3_fwd/v%d" % (4 if cin == 48 else 3), 2.0 * nv * 27 * cin * cout, nv * (cin + 2 * cout) * x.element_size() + 27 * cin * cout * 2,
                 lambda: _ck(lib().msseg_conv3d_k3_fwd_accumulate(_p(x), ld(x), _p(wp), _p(y), ld(y), N, D, H, W, cin, cout,
                                                                 _p(stats), _p(sc), sc.numel(), dt(x), _stream()),
                             "conv3d_k3_fwd_accumulate"))
    return y


def conv3d_k3_dgrad_inbwd(dy, wp, da, cin, cout, yraw, act, fwd_stats, slope, eps, dgamma=None, dbeta=None,
                          accumulate=False):
    """da = conv(dy, dgrad image) and, in the same launch, red[N][cout][2] = InstanceNorm-backward reductions of the
    layer (yraw, act, fwd_stats) that receives da.  Returns red."""
    _need_gpu(dy, wp, da, yraw, act, fwd_stats)
    N, D, H, W = dy.shape[:4]
    nv = N * D * H * W
    esz = dy.element_size()
    red = torch.empty(N, cout, 2, dtype=torch.float32, device=dy.device)
    sc = scratch(dy.device)

    def go():
        _ck(lib().msseg_conv3d_k3_dgrad_inbwd(_p(dy), ld(dy), _p(wp), _p(da), ld(da), N, D, H, W, cin, cout, _p(yraw),
                                              ld(yraw), _p(act), ld(act), _p(fwd_stats), slope, eps, _p(red),
                                              _p(dgamma), _p(dbeta), int(accumulate), _p(sc), sc.numel(), dt(dy),
                                              _stream()), "conv3d_k3_dgrad_inbwd")
    key = "conv3d_k3_fwd"
    if TIMER.enabled:
        key += "/v%d" % lib().msseg_conv3d_k3_kernel(N, D, H, W, cin, cout, dt(dy))
    TIMER.launch(key, 2.0 * nv * 27 * cin * cout, nv * (cin + 3 * cout) * esz + 27 * cin * cout * esz, go)
    return red


# --------------------------------------------------------------------------------------------
# conv k3 on small grids: split-K partials + a finish kernel that carries the rest of the unit (conv3d_k3_small.hip)
# --------------------------------------------------------------------------------------------
def conv3d_k3_small_ok(x, cin, cout) -> bool:
    """can the split-K small-grid path run conv k3 cin -> cout on a volume shaped like x ([N, D, H, W, C])?"""
    if os.environ.get("MSSEG_NO_K3_SMALL") or x.dim() != 5 or x.dtype != torch.bfloat16:
        return False
    N, D, H, W = x.shape[:4]
    return bool(lib().msseg_conv3d_k3_small_ok(N, D, H, W, cin, cout, BF16))


_k3s_ws = {}


def _k3s_workspace(nbytes, device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    buf = _k3s_ws.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        if buf is not None:
            _ws_retired.append(buf)       # captured graphs keep the old address
        buf = torch.empty(max(nbytes, 32 << 20) // 4, dtype=torch.float32, device=device)
        _k3s_ws[key] = buf
    return buf


def conv3d_k3_small_partials(x, wp, cin, cout):
    """(fp32 partial sums [stage groups][N * D * H * W][cout] of conv k3 (x, packed image with cout block 32), number of
    stage groups); the buffer is the module's grow-only scratch: consume it (a *_finish call) before the next partials
    call on the stream"""
    _need_gpu(x, wp)
    N, D, H, W = x.shape[:4]
    nv = N * D * H * W
    ng = lib().msseg_conv3d_k3_small_stage_groups(N, D, H, W, cin, cout)
    part = _k3s_workspace(lib().msseg_conv3d_k3_small_workspace_bytes(N, D, H, W, cin, cout), x.device)
    TIMER.launch("conv3d_k3_small", 2.0 * nv * 27 * cin * cout, nv * (cin * x.element_size() + ng * cout * 4) + 27 * cin * cout * 2,
                 lambda: _ck(lib().msseg_conv3d_k3_small_partials(_p(x), ld(x), _p(wp), _p(part), part.numel() * 4, N, D, H, W, cin,
                                                                  cout, _stream()), "conv3d_k3_small_partials"))
    return part, ng


def deconv_k2s2_small_unit_ok(dx_shape, cin, cout, dtype) -> bool:
    """can the input gradient of ConvTranspose3d k2 s2 (cin -> cout) for a coarse volume dx_shape = (N, D, H, W, cin) go out as a
    partial block for conv3d_k3_small_bwd_finish (which then runs the receiving unit's whole InstanceNorm backward)?"""
    if os.environ.get("MSSEG_NO_K3_SMALL") or dtype != torch.bfloat16 or len(dx_shape) != 5:
        return False
    N, D, H, W = dx_shape[:4]
    return N <= 8 and D * H * W <= 2048 and bool(lib().msseg_deconv_k2s2_bwd_partials_ok(cin, cout, BF16))


def deconv_k2s2_bwd_partials(dy, wp, cin, cout):
    """fp32 partial block [cin / 4][N * D * H * W][4] (ONE stage group) of the input gradient of ConvTranspose3d k2 s2; dy: fine
    [N, 2D, 2H, 2W, cout]; the buffer is the small-grid scratch: consume it (conv3d_k3_small_bwd_finish(part, 1, ...)) before
    the next partials call on the stream"""
    _need_gpu(dy, wp)
    N, D, H, W = dy.shape[0], dy.shape[1] // 2, dy.shape[2] // 2, dy.shape[3] // 2
    nv = N * D * H * W
    part = _k3s_workspace(nv * cin * 4, dy.device)
    TIMER.launch("deconv_k2s2_bwd_partials", 2.0 * nv * 8 * cin * cout, nv * (8 * cout * dy.element_size() + cin * 4) + 8 * cin * cout * 2,
                 lambda: _ck(lib().msseg_deconv_k2s2_bwd_partials(_p(dy), ld(dy), _p(wp), _p(part), part.numel() * 4, N, D, H, W, cin,
                                                                  cout, dt(dy), _stream()), "deconv_k2s2_bwd_partials"))
    return part


def conv3d_k3_small_fwd_finish(part, nstages, bias, gamma, beta, eps, slope, yraw, act, pooled, stats, residual=None):
    """residual (optional, same shape as act): act = lrelu(instance_norm(y) * gamma + beta + residual)"""
    _need_gpu(part, yraw, act, stats)
    N, D, H, W, cout = yraw.shape
    _ck(lib().msseg_conv3d_k3_small_fwd_finish(_p(part), nstages, _p(bias), _p(gamma), _p(beta), eps, slope, _p(yraw), ld(yraw),
                                               _p(act), ld(act), _p(residual), ld(residual) if residual is not None else 0,
                                               _p(pooled), ld(pooled) if pooled is not None else 0,
                                               _p(stats), N, D, H, W, cout, _stream()), "conv3d_k3_small_fwd_finish")


def conv3d_k3_small_bwd_finish(part, nstages, dx, unit=None, dgamma=None, dbeta=None, accumulate=False):
    """unit = (yraw, stats, gamma, beta, eps, slope) of the conv + InstanceNorm + LeakyReLU unit whose activation was the
    conv's input: dx then receives that unit's dy (and dgamma / dbeta its affine gradients); None: dx = the plain sum"""
    _need_gpu(part, dx)
    N, D, H, W, cin = dx.shape
    uy = ustats = ug = ub = None
    eps, slope = 1e-5, 1.0
    if unit is not None:
        uy, ustats, ug, ub, eps, slope = unit
    _ck(lib().msseg_conv3d_k3_small_bwd_finish(_p(part), nstages, _p(dx), ld(dx), _p(uy), ld(uy) if uy is not None else 0,
                                               _p(ustats), _p(ug), _p(ub), eps, slope, _p(dgamma), _p(dbeta),
                                               int(accumulate), N, D, H, W, cin, _stream()), "conv3d_k3_small_bwd_finish")
    return dx


def conv3d_k1_head(x, w, bias, y, cin, cout):
    """1x1x1 conv with 1..4 output channels straight from the fp32 weight [cout, cin] (streaming kernel)"""
    _need_gpu(x, w, y)
    nv = x.numel() // x.shape[-1]
    _ck(lib().msseg_conv3d_k1_head_fwd(_p(x), ld(x), _p(w), _p(bias), _p(y), ld(y), nv, cin, cout, dt(x), _stream()),
        "conv3d_k1_head_fwd")
    return y


def conv3d_k1_head_norm(yraw, stats, gamma, beta, slope, eps, w, bias, y, cin, cout):
    """y = conv1x1(lrelu(instance_norm(yraw))) for a head with <= 4 classes, normalisation applied on load"""
    _need_gpu(yraw, stats, w, y)
    N = yraw.shape[0]
    S = yraw.numel() // yraw.shape[-1] // N
    _ck(lib().msseg_conv3d_k1_head_norm_fwd(_p(yraw), ld(yraw), _p(stats), _p(gamma), _p(beta), slope, eps, _p(w), _p(bias),
                                            _p(y), ld(y), N, S, cin, cout, dt(yraw), _stream()), "conv3d_k1_head_norm_fwd")
    return y


def conv3d_k1_head_bwd_fused(dy, w, da, cin, cout, yraw, fwd_stats, gamma, beta, slope, eps, dw=None, dw_accumulate=False,
                             dgamma=None, dbeta=None, accumulate=False):
    """da = dy . w for a head with `cout` <= 4 classes (w fp32 [cout, cin]) and the InstanceNorm-backward sums of the layer
    (yraw, fwd_stats, gamma, beta) that receives da; with dw also the head's weight gradient dw[cout][cin] from the
    recomputed activation.  Returns red[N][cin][2].
    da None (dw given): the input gradient is not stored (the sums and dw are the same bits); instnorm_act_bwd_apply_head
    forms it again"""
    _need_gpu(dy, w, da, yraw, fwd_stats, dw)
    N = dy.shape[0]
    S = dy.numel() // dy.shape[-1] // N
    red = torch.empty(N, cin, 2, dtype=torch.float32, device=dy.device)
    sc = scratch(dy.device)
    _ck(lib().msseg_conv3d_k1_head_bwd_fused(_p(dy), ld(dy), _p(w), _p(da), ld(da) if da is not None else 0, N, S, cin, cout, _p(yraw), ld(yraw),
                                             _p(fwd_stats), _p(gamma), _p(beta), slope, eps, _p(red), _p(dgamma),
                                             _p(dbeta), int(accumulate), _p(dw), int(dw_accumulate), _p(sc), sc.numel(),
                                             dt(dy), _stream()), "conv3d_k1_head_bwd_fused")
    return red


def conv3d_k1(x, wp, bias, y, cin, cout):
    _need_gpu(x, wp, y)
    nv = x.numel() // x.shape[-1]
    _ck(lib().msseg_conv3d_k1_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(y), ld(y), nv, cin, cout, dt(x), _stream()),
        "conv3d_k1_fwd")
    return y


def conv3d_k1_dgrad_inbwd(dy, wp, da, cin, cout, yraw, act, fwd_stats, slope, eps, dgamma=None, dbeta=None,
                          accumulate=False):
    """da = dy @ W (1x1x1 input gradient, cin = channels of dy, cout = channels of da) + the InstanceNorm-backward sums of
    the layer (yraw, act, fwd_stats) that receives da, in one launch.  Returns red[N][cout][2]."""
    _need_gpu(dy, wp, da, yraw, act, fwd_stats)
    N = da.shape[0]
    S = da.numel() // (N * da.shape[-1])
    red = torch.empty(N, cout, 2, dtype=torch.float32, device=dy.device)
    sc = scratch(dy.device)
    _ck(lib().msseg_conv3d_k1_dgrad_inbwd(_p(dy), ld(dy), _p(wp), _p(da), ld(da), N, S, cin, cout, _p(yraw), ld(yraw),
                                          _p(act), ld(act), _p(fwd_stats), slope, eps, _p(red), _p(dgamma), _p(dbeta),
                                          int(accumulate), _p(sc), sc.numel(), dt(dy), _stream()), "conv3d_k1_dgrad_inbwd")
    return red


def deconv_k2s2_bwd_fused(dy, wp, dx, cin, cout, next_norm=None, dbias=None, dbias_accumulate=False, dgamma=None, dbeta=None,
                          accumulate=False):
    """dx of ConvTranspose3d k2 s2; next_norm = (yraw, act, fwd_stats, slope, eps) of the layer that receives dx adds its
    InstanceNorm-backward sums (returned as red[N][cin][2]); dbias (fp32 [cout]) receives the bias gradient."""
    _need_gpu(dy, wp, dx)
    N, D, H, W = dx.shape[:4]
    red = None
    yraw = act = stats = None
    slope = eps = 0.0
    if next_norm is not None:
        yraw, act, stats, slope, eps = next_norm
        red = torch.empty(N, cin, 2, dtype=torch.float32, device=dy.device)
    sc = scratch(dy.device)
    _ck(lib().msseg_deconv_k2s2_bwd_fused(_p(dy), ld(dy), _p(wp), _p(dx), ld(dx), N, D, H, W, cin, cout, _p(yraw),
                                          ld(yraw) if yraw is not None else 0, _p(act), ld(act) if act is not None else 0,
                                          _p(stats), slope, eps, _p(red), _p(dgamma), _p(dbeta), int(accumulate), _p(dbias),
                                          int(dbias_accumulate), _p(sc), sc.numel(), dt(dy), _stream()),
        "deconv_k2s2_bwd_fused")
    return red


def conv3d_gather(x, wp, bias, y, cin, cout, k, s, p):
    _need_gpu(x, wp, y)
    N, D, H, W = x.shape[:4]
    _ck(lib().msseg_conv3d_gather_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(y), ld(y), N, D, H, W, cin, cout, k, s, p,
                                      dt(x), _stream()), "conv3d_gather_fwd")
    return y


def conv3d_stem_norm(x, wp, bias, stats, gamma, beta, eps, slope, y, cout):
    """y = lrelu(instance_norm(conv k3 (x) + bias) * gamma + beta) of a ONE-channel volume with the statistics of a
    statistics-only conv3d_stem(x, ..., y=None, stats=...) call (inference: no raw output)"""
    _need_gpu(x, wp, y, stats)
    N, D, H, W = x.shape[:4]
    _ck(lib().msseg_conv3d_stem_norm_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(stats), _p(gamma), _p(beta), eps, slope, _p(y), ld(y),
                                         N, D, H, W, cout, dt(x), _stream()), "conv3d_stem_norm_fwd")
    return y


def conv3d_stem(x, wp, bias, y, cout, stats=None, k=3):
    """conv3d k3 p1 (k = 1: the 1x1x1 conv, image with K = 1) of a ONE-channel volume (bf16, cout % 32 == 0 or % 48 == 0) with
    optional fused InstanceNorm statistics; y None (with stats): statistics only"""
    _need_gpu(x, wp)
    N, D, H, W = x.shape[:4]
    sc = scratch(x.device) if stats is not None else None
    _ck(lib().msseg_conv3d_stem_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(y), ld(y) if y is not None else 0, N, D, H, W, cout,
                                    int(k), _p(stats), _p(sc), sc.numel() if sc is not None else 0, dt(x), _stream()),
        "conv3d_stem_fwd")
    return y


def deconv_k2s2(x, wp, bias, y, cin, cout):
    _need_gpu(x, wp, y)
    N, D, H, W = x.shape[:4]
    _ck(lib().msseg_deconv_k2s2_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(y), ld(y), N, D, H, W, cin, cout, dt(x),
                                    _stream()), "deconv_k2s2_fwd")
    return y


def deconv_k2s2_bwd_data(dy, wp, dx, cin, cout):
    _need_gpu(dy, wp, dx)
    N, D, H, W = dx.shape[:4]
    _ck(lib().msseg_deconv_k2s2_bwd_data(_p(dy), ld(dy), _p(wp), _p(dx), ld(dx), N, D, H, W, cin, cout, dt(dy),
                                         _stream()), "deconv_k2s2_bwd_data")
    return dx


def deconv_k4s4(x, wp, bias, y, cin, cout):
    """ConvTranspose3d k = s = 4: x [N,D,H,W,cin] -> y [N,4D,4H,4W,cout] (y may be a channel slice of a wider buffer)"""
    _need_gpu(x, wp, y)
    N, D, H, W = x.shape[:4]
    if tuple(y.shape) != (N, 4 * D, 4 * H, 4 * W, cout):
        raise ValueError(f"deconv_k4s4: output shape {tuple(y.shape)} for input {tuple(x.shape)}, cout {cout}")
    nv = N * D * H * W
    esz = x.element_size()
    TIMER.launch("deconv_k4s4_fwd", 2.0 * nv * 64 * cin * cout, nv * (cin + 64 * cout) * esz + 64 * cin * cout * esz,
                 lambda: _ck(lib().msseg_deconv_k4s4_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(y), ld(y), N, D, H, W, cin, cout,
                                                         dt(x), _stream()), "deconv_k4s4_fwd"))
    return y


def deconv_k4s4_bwd_data(dy, wp, dx, cin, cout):
    _need_gpu(dy, wp, dx)
    N, D, H, W = dx.shape[:4]
    if tuple(dy.shape) != (N, 4 * D, 4 * H, 4 * W, cout):
        raise ValueError(f"deconv_k4s4_bwd_data: gradient shape {tuple(dy.shape)} for input {tuple(dx.shape)}, cout {cout}")
    nv = N * D * H * W
    esz = dy.element_size()
    TIMER.launch("deconv_k4s4_bwd_data", 2.0 * nv * 64 * cin * cout, nv * (cin + 64 * cout) * esz + 64 * cin * cout * esz,
                 lambda: _ck(lib().msseg_deconv_k4s4_bwd_data(_p(dy), ld(dy), _p(wp), _p(dx), ld(dx), N, D, H, W, cin, cout,
                                                              dt(dy), _stream()), "deconv_k4s4_bwd_data"))
    return dx


# --------------------------------------------------------------------------------------------
# weight gradients
# --------------------------------------------------------------------------------------------
_ws_cache = {}
_ws_retired = []   # superseded workspaces: captured hipGraphs may still launch kernels against them, so they are never freed


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer per device.  A larger request allocates a new buffer; the old one is retired, not
    released, because graphs captured earlier keep its address baked into their kernel arguments."""
    key = (device.index if device.index is not None else torch.cuda.current_device())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)
        buf = torch.empty(max(nbytes, 64 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _wg_ws(M, T, K, device):
    return workspace(lib().msseg_wgrad_workspace_bytes(M, T, K), device)


def conv3d_k3_wgrad(x, dy, dw, cin, cout, accumulate=False):
    _need_gpu(x, dy, dw)
    N, D, H, W = x.shape[:4]
    ws = _wg_ws(cout, 27, cin, x.device)
    nv = N * D * H * W

    def go():
        _ck(lib().msseg_conv3d_k3_wgrad(_p(x), ld(x), _p(dy), ld(dy), _p(dw), N, D, H, W, cin, cout, int(accumulate),
                                        _p(ws), ws.numel(), dt(x), _stream()), "conv3d_k3_wgrad")
    key = "conv3d_k3_wgrad"
    if TIMER.enabled:
        key += "/v%d" % lib().msseg_conv3d_k3_wgrad_kernel(N, D, H, W, cin, cout, dt(x))
    TIMER.launch(key, 2.0 * nv * 27 * cin * cout, nv * (cin + cout) * x.element_size() + 27 * cin * cout * 4, go)


def conv3d_k1_wgrad(x, dy, dw, cin, cout, accumulate=False):
    _need_gpu(x, dy, dw)
    nv = x.numel() // x.shape[-1]
    ws = _wg_ws(cout, 1, cin, x.device)
    _ck(lib().msseg_conv3d_k1_wgrad(_p(x), ld(x), _p(dy), ld(dy), _p(dw), nv, cin, cout, int(accumulate), _p(ws),
                                    ws.numel(), dt(x), _stream()), "conv3d_k1_wgrad")


def linear_wgrad_ok(x, cin, cout) -> bool:
    return bool(x.is_cuda and x.dtype == torch.bfloat16 and
                lib().msseg_linear_wgrad_ok(x.numel() // x.shape[-1], cin, cout, BF16))


def linear_wgrad(x, dy, dw, dbias, cin, cout, accumulate_w=False, accumulate_b=False):
    """dw[cout][cin] (+)= dy^T x and dbias[cout] (+)= dy.sum(tokens) (dbias None: weight only) in one pass over the tokens"""
    _need_gpu(x, dy, dw)
    nv = x.numel() // x.shape[-1]
    ws = _wg_ws(cout, 1, cin, x.device)
    esz = x.element_size()
    TIMER.launch("linear_wgrad", 2.0 * nv * cin * cout, nv * (cin + cout) * esz + cin * cout * 4,
                 lambda: _ck(lib().msseg_linear_wgrad(_p(x), ld(x), _p(dy), ld(dy), _p(dw), _p(dbias), nv, cin, cout,
                                                      int(accumulate_w), int(accumulate_b), _p(ws), ws.numel(), dt(x),
                                                      _stream()), "linear_wgrad"))


def conv3d_gather_wgrad(x, dy, dw, cin, cout, k, s, p, accumulate=False):
    _need_gpu(x, dy, dw)
    N, D, H, W = x.shape[:4]
    ws = _wg_ws(cout, 1, cin * k ** 3, x.device)
    _ck(lib().msseg_conv3d_gather_wgrad(_p(x), ld(x), _p(dy), ld(dy), _p(dw), N, D, H, W, cin, cout, k, s, p,
                                        int(accumulate), _p(ws), ws.numel(), dt(x), _stream()), "conv3d_gather_wgrad")


def conv3d_stem_wgrad_inbwd_ok(x, y_raw, da, cout) -> bool:
    """can conv3d_stem_wgrad_inbwd take these operands (the one-channel stem kernels, 16-byte channel chunks, N <= 8)?"""
    return bool(x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] == 1 and x.shape[0] <= 8
                and (cout % 32 == 0 or cout % 48 == 0) and cout <= 256
                and all(ld(t) % 8 == 0 and t.data_ptr() % 16 == 0 for t in (y_raw, da)))


def conv3d_stem_wgrad_inbwd(x, y_raw, da, stats, red, gamma, beta, slope, eps, dw, cout, k=3, accumulate=False):
    """dw (+)= weight gradient of the one-input-channel conv (k 3 p 1, or k 1) from dy = the InstanceNorm + LeakyReLU backward
    apply of (y_raw, da, red), which is formed inside the kernel and never stored: the bits of instnorm_act_bwd_apply into a
    tensor followed by conv3d_gather_wgrad"""
    _need_gpu(x, y_raw, da, stats, red, dw)
    N, D, H, W = x.shape[:4]
    ws = _wg_ws(cout, 1, k ** 3, x.device)
    nv = N * D * H * W
    TIMER.launch("conv3d_stem_wgrad_inbwd", 2.0 * nv * cout * 27, nv * (2 * cout + 1) * 2 + cout * k ** 3 * 4,
                 lambda: _ck(lib().msseg_conv3d_stem_wgrad_inbwd(_p(x), ld(x), _p(y_raw), ld(y_raw), _p(da), ld(da), _p(stats),
                                                                 _p(red), _p(gamma), _p(beta), eps, slope, _p(dw), N, D, H, W,
                                                                 cout, k, int(accumulate), _p(ws), ws.numel(), dt(x),
                                                                 _stream()), "conv3d_stem_wgrad_inbwd"))


def deconv_k2s2_wgrad(x, dy, dw, cin, cout, accumulate=False):
    _need_gpu(x, dy, dw)
    N, D, H, W = x.shape[:4]
    ws = _wg_ws(cin, 1, 8 * cout, x.device)
    _ck(lib().msseg_deconv_k2s2_wgrad(_p(x), ld(x), _p(dy), ld(dy), _p(dw), N, D, H, W, cin, cout, int(accumulate),
                                      _p(ws), ws.numel(), dt(x), _stream()), "deconv_k2s2_wgrad")


def deconv_k4s4_wgrad(x, dy, dw, cin, cout, accumulate=False):
    """dw [cin, cout, 4,4,4] (+)= weight gradient of ConvTranspose3d k = s = 4; x coarse, dy fine (4x each way)"""
    _need_gpu(x, dy, dw)
    N, D, H, W = x.shape[:4]
    if tuple(dy.shape) != (N, 4 * D, 4 * H, 4 * W, cout) or dw.numel() != cin * cout * 64 or not dw.is_contiguous():
        raise ValueError(f"deconv_k4s4_wgrad: shapes x {tuple(x.shape)}, dy {tuple(dy.shape)}, dw {tuple(dw.shape)}")
    ws = _wg_ws(cin, 1, 64 * cout, x.device)
    nv = N * D * H * W
    TIMER.launch("deconv_k4s4_wgrad", 2.0 * nv * 64 * cin * cout, nv * (cin + 64 * cout) * x.element_size() + 64 * cin * cout * 4,
                 lambda: _ck(lib().msseg_deconv_k4s4_wgrad(_p(x), ld(x), _p(dy), ld(dy), _p(dw), N, D, H, W, cin, cout,
                                                           int(accumulate), _p(ws), ws.numel(), dt(x), _stream()),
                             "deconv_k4s4_wgrad"))


# --------------------------------------------------------------------------------------------
# norm / act / pool / layout
# --------------------------------------------------------------------------------------------
def _nsc(x):
    N, C = x.shape[0], x.shape[-1]
    return N, x.numel() // (N * C), C


def dwconv3d_k3(x, w_taps, bias, y, flip=False):
    """depthwise conv k3 p1 on channels-last x; w_taps [27, C] (tap-major, dtype of x); flip: the input gradient"""
    if w_taps.dtype != x.dtype:
        raise ValueError("dwconv3d_k3: the weight table must have the activation dtype")
    _need_gpu(x, w_taps, y)
    N, D, H, W, C = x.shape
    _ck(lib().msseg_dwconv3d_k3_fwd(_p(x), ld(x), _p(w_taps), _p(bias), _p(y), ld(y), N, D, H, W, C, int(flip), dt(x),
                                    _stream()), "dwconv3d_k3_fwd")
    return y


def avgpool3d_k3(x, y):
    """AvgPool3d(3, 1, 1) with count_include_pad: fp32 sum of the 27 taps x 1/27, one rounding"""
    _need_gpu(x, y)
    N, D, H, W, Cc = x.shape
    _ck(lib().msseg_avgpool3d_k3(_p(x), ld(x), _p(y), ld(y), N, D, H, W, Cc, dt(x), _stream()), "avgpool3d_k3")
    return y


def dwconv3d_k3_wgrad(x, dy, dw, dbias, acc_w=False, acc_b=False):
    """dw fp32 [C, 1, 3, 3, 3], dbias fp32 [C] (either may be None)"""
    _need_gpu(x, dy)
    N, D, H, W, C = x.shape
    sc = scratch(x.device)
    _ck(lib().msseg_dwconv3d_k3_wgrad(_p(x), ld(x), _p(dy), ld(dy), _p(dw), _p(dbias), int(acc_w), int(acc_b), N, D, H, W, C,
                                      _p(sc), sc.numel(), dt(x), _stream()), "dwconv3d_k3_wgrad")


def dwconv3d(x, w_taps, y, K, flip=False):
    """depthwise conv, odd K in 3..11, stride 1, pad K // 2, no bias, on channels-last x (a channel slice of a wider buffer is
    fine); w_taps [K^3, C] (tap-major, dtype of x); flip: the input gradient"""
    if w_taps.dtype != x.dtype or y.dtype != x.dtype:
        raise ValueError("dwconv3d: the weight table and the output must have the activation dtype")
    _need_gpu(x, w_taps, y)
    N, D, H, W, C = x.shape
    if tuple(w_taps.shape) != (K ** 3, C) or not w_taps.is_contiguous() or tuple(y.shape) != tuple(x.shape):
        raise ValueError(f"dwconv3d: weight table {tuple(w_taps.shape)} / output {tuple(y.shape)} do not fit x {tuple(x.shape)}, K {K}")
    _ck(lib().msseg_dwconv3d_fwd(_p(x), ld(x), _p(w_taps), _p(y), ld(y), N, D, H, W, C, K, int(flip), dt(x), _stream()),
        "dwconv3d_fwd")
    return y


def dwconv3d_wgrad(x, dy, dw, K, accumulate=False):
    """dw fp32 [C, 1, K, K, K] (+)= the weight gradient of dwconv3d; deterministic (fixed-order partial rows in the workspace)"""
    _need_gpu(x, dy, dw)
    N, D, H, W, C = x.shape
    if dw.dtype != torch.float32 or dw.numel() != C * K ** 3 or not dw.is_contiguous() or tuple(dy.shape) != tuple(x.shape):
        raise ValueError("dwconv3d_wgrad: dw must be contiguous fp32 [C, 1, K, K, K] and dy shaped like x")
    ws = workspace(lib().msseg_dwconv3d_wgrad_workspace_bytes(N, D, H, W, C, K, dt(x)), x.device)
    _ck(lib().msseg_dwconv3d_wgrad(_p(x), ld(x), _p(dy), ld(dy), _p(dw), int(accumulate), N, D, H, W, C, K, _p(ws), ws.numel(),
                                   dt(x), _stream()), "dwconv3d_wgrad")
    return dw


def focal_spatial_sum(x, out0, out1=None, g=None, m_in=None, scale=1.0, mode=0):
    """out0[n, c] = scale * sum over the voxels of x[n, ..., c] (* g[n, ..., 0], a one-channel view); mode 0 also writes
    out1 = GELU(out0), mode 1 multiplies by gelu'(m_in).  fp32 [N, C] results, fixed-order sums."""
    _need_gpu(x, out0)
    N, S, Cc = _nsc(x)
    sc = scratch(x.device)
    _ck(lib().msseg_focal_spatial_sum(_p(x), ld(x), _p(g), ld(g) if g is not None else 0, _p(m_in), _p(out0), _p(out1),
                                      float(scale), int(mode), N, S, Cc, _p(sc), sc.numel(), dt(x), _stream()),
        "focal_spatial_sum")
    return out0


def focal_aggregate_fwd(c1, c2, gates, gm, out):
    """out = c1 * g0 + c2 * g1 + gm[n, c] * g2; gates: a [..., >= 3] channel slice of a wider buffer; gm fp32 [N, C]"""
    _need_gpu(c1, c2, gates, gm, out)
    N, S, Cc = _nsc(c1)
    _ck(lib().msseg_focal_aggregate_fwd(_p(c1), _p(c2), _p(gates), ld(gates), _p(gm), _p(out), N, S, Cc, dt(c1), _stream()),
        "focal_aggregate_fwd")
    return out


def focal_aggregate_bwd(da, c1, c2, gates, gm, dmv, dc1, dc2, dgates):
    """dc1 = da * g0, dc2 = da * g1 + dmv[n, c], dgates[..., :3] = sum_c da * (c1, c2, gm), dgates[..., 3:] = 0"""
    _need_gpu(da, c1, c2, gates, gm, dmv, dc1, dc2, dgates)
    N, S, Cc = _nsc(c1)
    _ck(lib().msseg_focal_aggregate_bwd(_p(da), _p(c1), _p(c2), _p(gates), ld(gates), _p(gm), _p(dmv), _p(dc1), _p(dc2),
                                        _p(dgates), ld(dgates), dgates.shape[-1], N, S, Cc, dt(c1), _stream()),
        "focal_aggregate_bwd")


def focal_mul_fwd(q, h, y):
    """y = q * h; q may be a channel slice of a wider buffer"""
    _need_gpu(q, h, y)
    Cc = h.shape[-1]
    _ck(lib().msseg_focal_mul_fwd(_p(q), ld(q), _p(h), _p(y), h.numel() // Cc, Cc, dt(h), _stream()), "focal_mul_fwd")
    return y


def focal_mul_bwd(dy, q, h, dq, dh):
    """dq = dy * h (dq may be a channel slice of a wider buffer), dh = dy * q"""
    _need_gpu(dy, q, h, dq, dh)
    Cc = h.shape[-1]
    _ck(lib().msseg_focal_mul_bwd(_p(dy), _p(q), ld(q), _p(h), _p(dq), ld(dq), _p(dh), h.numel() // Cc, Cc, dt(h), _stream()),
        "focal_mul_bwd")


def interp_trilinear(x, y):
    """y = F.interpolate(x, size=y.shape[1:4], mode='trilinear', align_corners=False), both channels-last"""
    _need_gpu(x, y)
    N, ID, IH, IW, C = x.shape
    _ck(lib().msseg_interp_trilinear_fwd(_p(x), ld(x), _p(y), ld(y), N, ID, IH, IW, y.shape[1], y.shape[2], y.shape[3], C,
                                         dt(x), _stream()), "interp_trilinear_fwd")
    return y


def interp_trilinear_bwd(dy, dx):
    _need_gpu(dy, dx)
    N, ID, IH, IW, C = dx.shape
    OD, OH, OW = dy.shape[1:4]
    nb = lib().msseg_interp_trilinear_bwd_workspace_bytes(N, ID, IH, IW, OD, OH, OW, C)
    ws = torch.empty(nb, dtype=torch.uint8, device=dx.device)
    _ck(lib().msseg_interp_trilinear_bwd(_p(dy), ld(dy), _p(dx), ld(dx), N, ID, IH, IW, OD, OH, OW, C, _p(ws), nb, dt(dx),
                                         _stream()), "interp_trilinear_bwd")
    return dx


def kv_attention_fwd(q, kv, heads, scale):
    """q [B, N, C], kv [B, M, 2C] -> (o [B, N, C], lse [B, heads, N])"""
    _need_gpu(q, kv)
    B, N, C = q.shape
    M = kv.shape[1]
    o = torch.empty_like(q)
    lse = torch.empty(B, heads, N, dtype=torch.float32, device=q.device)
    _ck(lib().msseg_kv_attention_fwd(_p(q), _p(kv), _p(o), _p(lse), B, N, M, heads, C // heads, scale, dt(q), _stream()),
        "kv_attention_fwd")
    return o, lse


def kv_attention_bwd(q, kv, o, lse, dout, heads, scale):
    _need_gpu(q, kv, o, lse, dout)
    B, N, C = q.shape
    M = kv.shape[1]
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    nb = lib().msseg_kv_attention_bwd_workspace_bytes(B, N, M, heads, C // heads)
    ws = torch.empty(nb, dtype=torch.uint8, device=q.device)
    _ck(lib().msseg_kv_attention_bwd(_p(q), _p(kv), _p(o), _p(lse), _p(dout), _p(dq), _p(dkv), B, N, M, heads, C // heads,
                                     scale, _p(ws), nb, dt(q), _stream()), "kv_attention_bwd")
    return dq, dkv


def scale_channels(x, scale, y):
    """y[n, ..., c] = x[n, ..., c] * scale[n, c] (fp32 scale)"""
    _need_gpu(x, scale, y)
    N, C = x.shape[0], x.shape[-1]
    _ck(lib().msseg_scale_channels(_p(x), _p(scale), _p(y), N, x.numel() // (N * C), C, dt(x), _stream()), "scale_channels")
    return y


def channel_stats(x, stats=None):
    _need_gpu(x)
    N, S, Cc = _nsc(x)
    if stats is None:
        stats = torch.empty(N, Cc, 2, dtype=torch.float32, device=x.device)
    sc = scratch(x.device)
    _ck(lib().msseg_channel_stats(_p(x), ld(x), _p(stats), N, S, Cc, _p(sc), sc.numel(), dt(x), _stream()),
        "channel_stats")
    return stats


def instnorm_act_fwd(x, stats, gamma, beta, y, slope, eps=1e-5, residual=None):
    _need_gpu(x, stats, y)
    N, S, Cc = _nsc(x)
    TIMER.launch("instnorm_act_fwd", 0.0, _nbytes(x, y, residual), lambda: _ck(lib().msseg_instnorm_act_fwd(_p(x), ld(x), _p(stats), _p(gamma), _p(beta), _p(residual),
                                     ld(residual) if residual is not None else 0, _p(y), ld(y), N, S, Cc, eps, slope,
                                     dt(x), _stream()), "instnorm_act_fwd"))
    return y


def instnorm_pool_ok(x, y, pooled) -> bool:
    """the fused InstanceNorm + LeakyReLU + MaxPool3d(2) kernel wants even spatial sizes and 16-byte channel chunks"""
    epc = 16 // x.element_size()
    return (x.dim() == 5 and all(int(d) % 2 == 0 for d in x.shape[1:4]) and x.shape[-1] % epc == 0
            and all(ld(t) % epc == 0 and t.data_ptr() % 16 == 0 for t in (x, y, pooled)))


def instnorm_act_pool_fwd(x, stats, gamma, beta, y, pooled, slope, eps=1e-5):
    """y = lrelu(instance_norm(x)) and pooled = max_pool3d(y, 2) in one pass over x (channels-last [N, D, H, W, C])"""
    _need_gpu(x, stats, y, pooled)
    N, D, H, W, Cc = x.shape
    TIMER.launch("instnorm_act_pool_fwd", 0.0, _nbytes(x, y, pooled), lambda: _ck(lib().msseg_instnorm_act_pool_fwd(_p(x), ld(x), _p(stats), _p(gamma), _p(beta), _p(y), ld(y), _p(pooled), ld(pooled),
                                          N, D, H, W, Cc, eps, slope, dt(x), _stream()), "instnorm_act_pool_fwd"))
    return y, pooled


def instnorm_act_poolbwd_reduce(x, stats, gamma, beta, skip, g, da, slope, eps=1e-5, dgamma=None, dbeta=None,
                                accumulate=False):
    """da = skip + max_pool3d-backward(lrelu(instance_norm(x)), g) (dense) and the InstanceNorm-backward sums of da;
    returns red[N][C][2].  Follow with instnorm_act_bwd_apply(x, ..., dy=da, red)."""
    _need_gpu(x, stats, skip, g, da)
    N, D, H, W, Cc = x.shape
    red = torch.empty(N, Cc, 2, dtype=torch.float32, device=x.device)
    sc = scratch(x.device)
    TIMER.launch("instnorm_act_poolbwd_reduce", 0.0, _nbytes(x, skip, g, da), lambda: _ck(lib().msseg_instnorm_act_poolbwd_reduce(_p(x), ld(x), _p(stats), _p(gamma), _p(beta), _p(skip), ld(skip), _p(g),
                                                ld(g), _p(da), ld(da), _p(red), _p(dgamma), _p(dbeta), int(accumulate),
                                                N, D, H, W, Cc, eps, slope, _p(sc), sc.numel(), dt(x), _stream()),
        "instnorm_act_poolbwd_reduce"))
    return red


def instnorm_act_bwd(x, stats, gamma, y, dy, dx, slope, eps=1e-5, dres=None, dgamma=None, dbeta=None,
                     accumulate=False, beta=None):
    """dx (and dres) from dy; the affine gradients dgamma/dbeta (fp32 [C]) are written (or accumulated) by the
    reduce kernel's finalising block.  Returns red[N][C][2] = (sum dz, sum dz*xhat)."""
    _need_gpu(x, stats, dy, dx)
    red = instnorm_act_bwd_reduce(x, stats, gamma, y, dy, slope, eps, dgamma, dbeta, accumulate, beta)
    instnorm_act_bwd_apply(x, stats, gamma, y, dy, red, dx, slope, eps, dres, beta)
    return red


def instnorm_act_bwd_reduce(x, stats, gamma, y, dy, slope, eps=1e-5, dgamma=None, dbeta=None, accumulate=False, beta=None):
    """first half of instnorm_act_bwd: red[N][C][2] = (sum dz, sum dz*xhat) (+ dgamma / dbeta)"""
    _need_gpu(x, stats, dy)
    N, S, Cc = _nsc(x)
    red = torch.empty(N, Cc, 2, dtype=torch.float32, device=x.device)
    sc = scratch(x.device)
    TIMER.launch("instnorm_act_bwd_reduce", 0.0, _nbytes(x, y, dy), lambda: _ck(lib().msseg_instnorm_act_bwd_reduce(_p(x), ld(x), _p(stats), _p(gamma), _p(beta), _p(y),
                                            ld(y) if y is not None else 0, _p(dy), ld(dy), _p(red),
                                            _p(dgamma), _p(dbeta), int(accumulate), N, S, Cc, eps, slope, _p(sc),
                                            sc.numel(), dt(x), _stream()), "instnorm_act_bwd_reduce"))
    return red


def instnorm_act_bwd_apply(x, stats, gamma, y, dy, red, dx, slope, eps=1e-5, dres=None, beta=None):
    """y None: the sign of the pre-activation is recomputed from x (layers without residual)"""
    _need_gpu(x, stats, dy, dx, red)
    N, S, Cc = _nsc(x)
    TIMER.launch("instnorm_act_bwd_apply", 0.0, _nbytes(x, y, dy, dx, dres), lambda: _ck(lib().msseg_instnorm_act_bwd_apply(_p(x), ld(x), _p(stats), _p(gamma), _p(beta), _p(y),
                                           ld(y) if y is not None else 0, _p(dy), ld(dy), _p(red),
                                           _p(dx), ld(dx), _p(dres), ld(dres) if dres is not None else 0, N, S, Cc, eps,
                                           slope, dt(x), _stream()), "instnorm_act_bwd_apply"))
    return red


def instnorm_act_bwd_apply_head(x, stats, gamma, beta, dl, w, cout, red, dx, slope, eps=1e-5):
    """instnorm_act_bwd_apply (y None, no dres) with the gradient of the activation formed from the class gradient rows dl
    ([..., 16 bytes]) and the head's weight w (fp32 [cout, C]) instead of read from a tensor: the bits of the plain apply fed
    with the da that conv3d_k1_head_bwd_fused stores"""
    _need_gpu(x, stats, dl, w, red, dx)
    N, S, Cc = _nsc(x)
    TIMER.launch("instnorm_act_bwd_apply_head", 8.0 * N * S * Cc, _nbytes(x, dl, dx),
                 lambda: _ck(lib().msseg_instnorm_act_bwd_apply_head(_p(x), ld(x), _p(stats), _p(gamma), _p(beta), _p(dl), ld(dl),
                                                                     _p(w), cout, _p(red), _p(dx), ld(dx), N, S, Cc, eps, slope,
                                                                     dt(x), _stream()), "instnorm_act_bwd_apply_head"))
    return dx


def maxpool2_fwd(x, y):
    _need_gpu(x, y)
    N, D, H, W, Cc = x.shape
    _ck(lib().msseg_maxpool2_fwd(_p(x), ld(x), _p(y), ld(y), N, D, H, W, Cc, dt(x), _stream()), "maxpool2_fwd")
    return y


def maxpool2_bwd(x, dy, dx, accumulate=False):
    _need_gpu(x, dy, dx)
    N, D, H, W, Cc = x.shape
    _ck(lib().msseg_maxpool2_bwd(_p(x), ld(x), _p(dy), ld(dy), _p(dx), ld(dx), N, D, H, W, Cc, int(accumulate), dt(x),
                                 _stream()), "maxpool2_bwd")
    return dx


def to_channels_last(src: torch.Tensor, dst: torch.Tensor):
    """src NCDHW contiguous -> dst [N, D, H, W, C] (dtype cast included)."""
    _need_gpu(src, dst)
    src = src.contiguous()
    N, Cc = src.shape[0], src.shape[1]
    S = src.numel() // (N * Cc)
    _ck(lib().msseg_ncdhw_to_ndhwc(_p(src), dt(src), _p(dst), ld(dst), dt(dst), N, Cc, S, _stream()), "ncdhw_to_ndhwc")
    return dst


def to_channels_first(src: torch.Tensor, dst: torch.Tensor):
    """src [N, D, H, W, C] (view allowed) -> dst NCDHW contiguous."""
    _need_gpu(src, dst)
    N, Cc = dst.shape[0], dst.shape[1]
    S = dst.numel() // (N * Cc)
    assert dst.is_contiguous()
    _ck(lib().msseg_ndhwc_to_ncdhw(_p(src), ld(src), dt(src), _p(dst), dt(dst), N, Cc, S, _stream()), "ndhwc_to_ncdhw")
    return dst


def channel_sum(x, out, accumulate=False):
    _need_gpu(x, out)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    sc = scratch(x.device)
    _ck(lib().msseg_channel_sum(_p(x), ld(x), _p(out), rows, Cc, int(accumulate), _p(sc), sc.numel(), dt(x),
                                _stream()), "channel_sum")
    return out


def axpy_rows(a, b, scale, y):
    """y[n] = a[n] + scale[n] * b[n] (a None: scale * b; scale None: plain add) on dense tensors [N, ...]"""
    _need_gpu(b, y)
    assert b.is_contiguous() and y.is_contiguous() and (a is None or a.is_contiguous())
    N = b.shape[0]
    _ck(lib().msseg_axpy_rows(_p(a), _p(b), _p(scale), _p(y), N, b.numel() // N, dt(b), _stream()), "axpy_rows")
    return y


def add(a, b, y):
    _need_gpu(a, b, y)
    Cc = a.shape[-1]
    rows = a.numel() // Cc
    _ck(lib().msseg_add(_p(a), ld(a), _p(b), ld(b), _p(y), ld(y), rows, Cc, dt(a), _stream()), "add")
    return y


# --------------------------------------------------------------------------------------------
# loss / metric
# --------------------------------------------------------------------------------------------
# loss kinds of the seg_loss_* passes (MSSEG_LOSS_* of include/msseg.h)
LOSS_DICE_CE, LOSS_TVERSKY, LOSS_DICE_FOCAL = 0, 1, 2


MAX_REGIONS = 16


def region_masks(masks, n_regions=None):
    """the msseg_region_masks image (16 uint32) of a tuple of region bit masks, for the msseg_region_* entry points"""
    masks = tuple(int(m) for m in masks)
    if not 1 <= len(masks) <= MAX_REGIONS or (n_regions is not None and len(masks) != n_regions):
        raise ValueError(f"a region table holds 1..{MAX_REGIONS} masks, one per logits channel: got {len(masks)}"
                         + (f" for {n_regions} channels" if n_regions is not None else ""))
    if any(m < 0 or m >= 1 << 32 for m in masks):
        raise ValueError("region masks are uint32 bit sets of the label values 0..31")
    return (C.c_uint32 * 16)(*masks)


def seg_loss_partials(logits, labels, n_cls, kind, channels_last_ld=0, want_hard=False, regions=None):
    """atomic partial sums (any N) for a loss kind: slot 1 / slot 3 of partial hold (sum p^2, CE sum) | (sum p, 0) | (sum p^2, focal sum).
    logits: NCDHW (channels_last_ld == 0) or channels-last with voxel stride ld.  Returns (partial, hard).
    regions (here and in the three passes below): a tuple of n_cls region bit masks selects the sigmoid form of the kind
    (msseg_region_loss_*: the target of channel c is bit `label` of regions[c])."""
    _need_gpu(logits, labels)
    N = logits.shape[0]
    S = labels.numel() // N
    partial = torch.zeros(N, n_cls, 4, dtype=torch.float32, device=logits.device)
    hard = torch.zeros(N, n_cls, 3, dtype=torch.float32, device=logits.device) if want_hard else None
    if regions is not None:
        _ck(lib().msseg_region_loss_partials(_p(logits), channels_last_ld, dt(logits), _p(labels), _LAB[labels.dtype],
                                             _p(partial), _p(hard), N, S, n_cls, kind, region_masks(regions, n_cls),
                                             _stream()), "region_loss_partials")
        return partial, hard
    _ck(lib().msseg_seg_loss_partials(_p(logits), channels_last_ld, dt(logits), _p(labels), _LAB[labels.dtype],
                                      _p(partial), _p(hard), N, S, n_cls, kind, _stream()), "seg_loss_partials")
    return partial, hard


def seg_loss_fwd(logits, labels, n_cls, smooth_nr, smooth_dr, kind, alpha=0.0, beta=0.0, channels_last_ld=0, want_hard=True,
                 regions=None):
    """deterministic fused forward (N <= 8): (partial [N,C,4], hard [N,C,3] or None, loss3 = (total, first term, second term))"""
    _need_gpu(logits, labels)
    N = logits.shape[0]
    S = labels.numel() // N
    partial = torch.empty(N, n_cls, 4, dtype=torch.float32, device=logits.device)
    hard = torch.empty(N, n_cls, 3, dtype=torch.float32, device=logits.device) if want_hard else None
    loss = torch.empty(3, dtype=torch.float32, device=logits.device)
    sc = scratch(logits.device)
    if regions is not None:
        _ck(lib().msseg_region_loss_fwd(_p(logits), channels_last_ld, dt(logits), _p(labels), _LAB[labels.dtype], _p(partial),
                                        _p(hard), _p(loss), N, S, n_cls, smooth_nr, smooth_dr, kind, alpha, beta,
                                        region_masks(regions, n_cls), _p(sc), sc.numel(), _stream()), "region_loss_fwd")
        return partial, hard, loss
    _ck(lib().msseg_seg_loss_fwd(_p(logits), channels_last_ld, dt(logits), _p(labels), _LAB[labels.dtype], _p(partial),
                                 _p(hard), _p(loss), N, S, n_cls, smooth_nr, smooth_dr, kind, alpha, beta, _p(sc),
                                 sc.numel(), _stream()), "seg_loss_fwd")
    return partial, hard, loss


def seg_loss_finalize(partial, S, smooth_nr, smooth_dr, kind, alpha=0.0, beta=0.0, regions=None):
    N, Cc = partial.shape[0], partial.shape[1]
    loss = torch.empty(3, dtype=torch.float32, device=partial.device)
    if regions is not None:
        _ck(lib().msseg_region_loss_finalize(_p(partial), _p(loss), N, S, Cc, smooth_nr, smooth_dr, kind, alpha, beta,
                                             _stream()), "region_loss_finalize")
        return loss
    _ck(lib().msseg_seg_loss_finalize(_p(partial), _p(loss), N, S, Cc, smooth_nr, smooth_dr, kind, alpha, beta, _stream()),
        "seg_loss_finalize")
    return loss


def seg_loss_bwd(logits, labels, partial, gscale, dlogits, n_cls, smooth_nr, smooth_dr, kind, alpha=0.0, beta=0.0, ld_in=0,
                 ld_out=0, regions=None):
    _need_gpu(logits, labels, partial, dlogits)
    N = logits.shape[0]
    S = labels.numel() // N
    if regions is not None:
        _ck(lib().msseg_region_loss_bwd(_p(logits), ld_in, dt(logits), _p(labels), _LAB[labels.dtype], _p(partial),
                                        _p(gscale), _p(dlogits), ld_out, N, S, n_cls, smooth_nr, smooth_dr, kind, alpha, beta,
                                        region_masks(regions, n_cls), _stream()), "region_loss_bwd")
        return dlogits
    _ck(lib().msseg_seg_loss_bwd(_p(logits), ld_in, dt(logits), _p(labels), _LAB[labels.dtype], _p(partial), _p(gscale),
                                 _p(dlogits), ld_out, N, S, n_cls, smooth_nr, smooth_dr, kind, alpha, beta, _stream()),
        "seg_loss_bwd")
    return dlogits


# --------------------------------------------------------------------------------------------
# optimiser
# --------------------------------------------------------------------------------------------
def adamw_step(param, grad, exp_avg, exp_avg_sq, decay_mask, lr, beta1, beta2, eps, weight_decay, step,
               grad_scale=None, dev_hyper=None):
    _need_gpu(param, grad, exp_avg, exp_avg_sq)
    _ck(lib().msseg_adamw_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(decay_mask), param.numel(), lr,
                               beta1, beta2, eps, weight_decay, step, _p(grad_scale), _p(dev_hyper), _stream()),
        "adamw_step")


def sumsq(x, out, partials):
    """out[0] = sum of x^2 in a fixed order; `partials`: fp32 buffer of the caller for the per-block sums (overwritten)."""
    _need_gpu(x, out, partials)
    if partials.dtype != torch.float32 or not partials.is_contiguous():
        raise ValueError("sumsq: partials must be a contiguous fp32 buffer")
    _ck(lib().msseg_sumsq(_p(x), x.numel(), _p(out), _p(partials), partials.numel(), _stream()), "sumsq")
    return out


# --------------------------------------------------------------------------------------------
# sliding window
# --------------------------------------------------------------------------------------------
def sw_normalize(out, cnt):
    _need_gpu(out, cnt)
    _ck(lib().msseg_sw_normalize(_p(out), _p(cnt), out.shape[0], cnt.numel(), _stream()), "sw_normalize")
    return out


def _sw_flips(flips, table, nwin):
    """the optional per-row mirror masks of the batched sliding-window calls: device int32 [>= nwin] next to `table`"""
    if flips is None:
        return None
    _need_gpu(flips)
    if flips.dtype != torch.int32 or not flips.is_contiguous() or flips.dim() != 1 or flips.shape[0] < nwin \
            or flips.device != table.device:
        raise ValueError("flips: contiguous int32 [>= nwin] on the table's device")
    return flips


def sw_gather_batch(vol, win, table, nwin, cval=0.0, channels_last_ld=0, flips=None):
    """vol: [B, C, *vol] fp32 ; win: [nwin, C, *roi] (ld 0) or channels-last [nwin, *roi, ld] ; table: int32 [>=nwin, 4]
    device tensor of (b, z0, y0, x0), b < 0 = unused slot.  flips: optional int32 [>=nwin] device tensor, bit 0 / 1 / 2 =
    row j's window is mirrored along D / H / W (torch.flip of the plain window)."""
    _need_gpu(vol, win, table)
    flips = _sw_flips(flips, table, nwin)
    assert vol.dtype == torch.float32 and vol.is_contiguous() and win.is_contiguous()
    assert table.dtype == torch.int32 and table.is_contiguous() and table.shape[0] >= nwin
    Cc = vol.shape[1]
    VD, VH, VW = vol.shape[2:]
    RD, RH, RW = win.shape[2:] if channels_last_ld == 0 else win.shape[1:4]
    _ck(lib().msseg_sw_gather_batch(_p(vol), vol.stride(0), _p(win), channels_last_ld, dt(win), _p(table), _p(flips), nwin,
                                    Cc, VD, VH, VW, RD, RH, RW, float(cval), _stream()), "sw_gather_batch")
    return win


def sw_blend_batch(win, imp, out, cnt, table, nwin, channels_last_ld=0, flips=None):
    """out: [B, C, *vol] fp32 ; cnt: [B, *vol] fp32 ; win as in sw_gather_batch (C = out.shape[1] channels used).
    flips: as in sw_gather_batch -- row j's logits are un-mirrored on the way in, `imp` stays in volume orientation."""
    _need_gpu(win, imp, out, cnt, table)
    flips = _sw_flips(flips, table, nwin)
    assert out.is_contiguous() and cnt.is_contiguous() and win.is_contiguous() and imp.is_contiguous()
    assert table.dtype == torch.int32 and table.is_contiguous() and table.shape[0] >= nwin
    Cc = out.shape[1]
    VD, VH, VW = out.shape[2:]
    RD, RH, RW = imp.shape
    _ck(lib().msseg_sw_blend_batch(_p(win), channels_last_ld, dt(win), _p(imp), _p(out), out.stride(0), _p(cnt),
                                   cnt.stride(0), _p(table), _p(flips), nwin, Cc, VD, VH, VW, RD, RH, RW, _stream()),
        "sw_blend_batch")


# --------------------------------------------------------------------------------------------
# post-inference
# --------------------------------------------------------------------------------------------
def argmax_u8(logits: torch.Tensor) -> torch.Tensor:
    """logits [C, D, H, W] fp32 (one sample, contiguous) -> uint8 [D, H, W], first maximum over C"""
    _need_gpu(logits)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 4
    out = torch.empty(logits.shape[1:], dtype=torch.uint8, device=logits.device)
    _ck(lib().msseg_argmax_u8(_p(logits), logits.shape[0], out.numel(), _p(out), _stream()), "argmax_u8")
    return out


def region_decode_u8(logits: torch.Tensor, values, want_bits: bool = False):
    """sigmoid logits [C, D, H, W] fp32 (one sample, contiguous) -> uint8 [D, H, W]: 0, then values[c] for every channel c in
    order whose logit is > 0 (later regions paint over earlier ones; NaN does not fire).  want_bits: also the uint16 map of
    the fired channels (bit c), returned as (map, bits)."""
    _need_gpu(logits)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 4
    values = tuple(int(v) for v in values)
    if len(values) != logits.shape[0] or any(v < 0 or v > 255 for v in values):
        raise ValueError(f"region_decode_u8: one value in 0..255 per channel ({logits.shape[0]}), got {values!r}")
    out = torch.empty(logits.shape[1:], dtype=torch.uint8, device=logits.device)
    bits = torch.empty(logits.shape[1:], dtype=torch.uint16, device=logits.device) if want_bits else None
    _ck(lib().msseg_region_decode_u8(_p(logits), logits.shape[0], out.numel(), (C.c_uint8 * 16)(*values), _p(out), _p(bits),
                                     _stream()), "region_decode_u8")
    return (out, bits) if want_bits else out


def region_counts_u8(pred: torch.Tensor, label: torch.Tensor, masks) -> torch.Tensor:
    """two uint8 label maps of the same voxel count -> float32 [R, 3] = (|P_r & T_r|, |P_r|, |T_r|) per region r, both maps
    taken through the region bit masks; integer sums in a fixed order"""
    _need_gpu(pred, label)
    assert pred.dtype == torch.uint8 and label.dtype == torch.uint8 and pred.is_contiguous() and label.is_contiguous()
    assert pred.numel() == label.numel(), "prediction and label differ in voxel count"
    rm = region_masks(masks)
    counts = torch.empty(len(masks), 3, dtype=torch.float32, device=pred.device)
    sc = scratch(pred.device)
    _ck(lib().msseg_region_counts_u8(_p(pred), _p(label), pred.numel(), len(masks), rm, _p(counts), _p(sc), sc.numel(),
                                     _stream()), "region_counts_u8")
    return counts


def resample_nearest_u8(src: torch.Tensor, target_size) -> torch.Tensor:
    """uint8 [D, H, W] -> uint8 target_size, scipy.ndimage.zoom(order=0) semantics"""
    _need_gpu(src)
    assert src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 3
    td, th, tw = (int(v) for v in target_size)
    out = torch.empty(td, th, tw, dtype=torch.uint8, device=src.device)
    _ck(lib().msseg_resample_nearest_u8(_p(src), src.shape[0], src.shape[1], src.shape[2], _p(out), td, th, tw, _stream()),
        "resample_nearest_u8")
    return out


def majority_vote_u8(labels: torch.Tensor, n_classes: int) -> torch.Tensor:
    """labels [F, D, H, W] uint8 (one label map per fold) -> uint8 [D, H, W]"""
    _need_gpu(labels)
    assert labels.dtype == torch.uint8 and labels.is_contiguous() and labels.dim() >= 2
    out = torch.empty(labels.shape[1:], dtype=torch.uint8, device=labels.device)
    _ck(lib().msseg_majority_vote_u8(_p(labels), labels.shape[0], out.numel(), n_classes, _p(out), _stream()),
        "majority_vote_u8")
    return out


class RestoreDesc(C.Structure):
    """mirror of msseg_restore_desc (include/msseg.h); data_device.restore_descriptor builds it from a record"""
    _fields_ = [("native", C.c_int32 * 3), ("perm", C.c_int32 * 3), ("flip", C.c_int32 * 3), ("grid", C.c_int32 * 3),
                ("offset", C.c_int32 * 3), ("model", C.c_int32 * 3), ("scale", C.c_double * 3)]


def restore_native_u8(src: torch.Tensor, desc_or_record, mode: str = "nearest") -> torch.Tensor:
    """A prediction on the model grid -> uint8 [native], the grid of the file array: the inverse of
    data_device.preprocess_volume (pad, foreground crop, spacing resample, RAS reorientation) in one launch.
    mode "nearest": src uint8 [D, H, W], a label map.  mode "linear": src fp32 [C, D, H, W], logits; they are resampled
    trilinearly and the first arg max is taken per native voxel, without forming [C, native].  Voxels the foreground crop
    removed are class 0.  desc_or_record: a RestoreDesc or anything data_device.restore_descriptor accepts.  Allocates the
    output only."""
    if mode not in ("nearest", "linear"):
        raise ValueError(f"restore_native_u8: mode {mode!r}: 'nearest' or 'linear'")
    _need_gpu(src)
    if isinstance(desc_or_record, RestoreDesc):
        desc = desc_or_record
    else:
        from .data_device import restore_descriptor
        desc = restore_descriptor(desc_or_record)
    logits = mode == "linear"
    assert src.is_contiguous() and src.dtype == (torch.float32 if logits else torch.uint8) and src.dim() == (4 if logits else 3), \
        "restore_native_u8: src must be a contiguous uint8 [D, H, W] (nearest) or fp32 [C, D, H, W] (linear) tensor"
    if tuple(src.shape[-3:]) != tuple(desc.model):
        raise ValueError(f"restore_native_u8: src's grid {tuple(src.shape[-3:])} is not the descriptor's {tuple(desc.model)}")
    # the entry point validates the descriptor and names what is wrong with it; a negative length only has to get that far
    out = torch.empty([max(int(v), 0) for v in desc.native], dtype=torch.uint8, device=src.device)
    _ck(lib().msseg_restore_native_u8(_p(src), int(logits), int(src.shape[0]) if logits else 0, C.addressof(desc), _p(out),
                                      _stream()), "restore_native_u8")
    return out


def hd_edges(pred: torch.Tensor, gt: torch.Tensor, n_classes: int):
    """pred / gt: uint8 label maps [D, H, W] -> (edge map of pred, edge map of gt, stats int32 [n_classes, 8])"""
    _need_gpu(pred, gt)
    assert pred.dtype == torch.uint8 and gt.dtype == torch.uint8 and pred.shape == gt.shape and pred.dim() == 3
    pred, gt = pred.contiguous(), gt.contiguous()
    D, H, W = pred.shape
    ep, eg = torch.empty_like(pred), torch.empty_like(gt)
    stats = torch.empty(n_classes, 8, dtype=torch.int32, device=pred.device)
    _ck(lib().msseg_hd_edges(_p(pred), _p(gt), D, H, W, n_classes, _p(ep), _p(eg), _p(stats), _stream()), "hd_edges")
    return ep, eg, stats


def hd_directed_hist(edges_src, edges_tgt, cls: int, box, hist: torch.Tensor):
    """histogram (int32, on the device) of the squared distances from the class-`cls` surface voxels of edges_tgt to the
    nearest class-`cls` surface voxel of edges_src inside box = (z0, y0, x0, z1, y1, x1); the last bin counts 'no source'"""
    _need_gpu(edges_src, edges_tgt, hist)
    D, H, W = edges_src.shape
    bz, by, bx = box[3] - box[0], box[4] - box[1], box[5] - box[2]
    ws = workspace(lib().msseg_hd_directed_workspace_bytes(bz, by, bx), edges_src.device)
    b6 = (C.c_int * 6)(*[int(v) for v in box])
    _ck(lib().msseg_hd_directed_hist(_p(edges_src), _p(edges_tgt), int(cls), D, H, W, b6, _p(ws), ws.numel(), _p(hist),
                                     hist.numel(), _stream()), "hd_directed_hist")
    return hist


def sd_directed_mm(edges_src, edges_tgt, cls: int, box, spacing, workspace_bytes: Optional[int] = None):
    """float64 map [bz, by, bx] over box = (z0, y0, x0, z1, y1, x1): the squared distance in physical units (spacing: three
    floats, one per tensor axis) from every class-`cls` surface voxel of edges_tgt to the nearest class-`cls` surface voxel of
    edges_src (+inf when edges_src has none), -1 at every other voxel.  workspace_bytes: pass less than the entry point needs
    (for its refusal); default: what it needs."""
    _need_gpu(edges_src, edges_tgt)
    assert edges_src.dtype == torch.uint8 and edges_tgt.dtype == torch.uint8 and edges_src.dim() == 3 and \
        edges_src.shape == edges_tgt.shape and edges_src.is_contiguous() and edges_tgt.is_contiguous()
    D, H, W = edges_src.shape
    box = [int(v) for v in box]
    bz, by, bx = box[3] - box[0], box[4] - box[1], box[5] - box[2]
    need = lib().msseg_sd_directed_workspace_bytes(max(bz, 0), max(by, 0), max(bx, 0))
    ws = workspace(need, edges_src.device)
    # the entry point validates the box and names what is wrong with it; a negative extent only has to get that far
    out = torch.empty(max(bz, 0), max(by, 0), max(bx, 0), dtype=torch.float64, device=edges_src.device)
    b6 = (C.c_int * 6)(*box)
    s3 = (C.c_double * 3)(*[float(v) for v in spacing])
    _ck(lib().msseg_sd_directed_mm(_p(edges_src), _p(edges_tgt), int(cls), D, H, W, b6, s3, _p(ws),
                                   ws.numel() if workspace_bytes is None else int(workspace_bytes), _p(out), _stream()),
        "sd_directed_mm")
    return out


class SurfaceSummary(NamedTuple):
    n: int                       # surface voxels (entries >= 0 of the map)
    n_inf: int                   # of them: +inf
    sum: float                   # sum of sqrt(d2) over the finite ones
    within: np.ndarray           # int64 [len(tolerances)]: entries with sqrt(d2) <= tolerance
    d2_at_rank: np.ndarray       # float64 [len(ranks)]: order statistics of d2 (NaN: rank past the last entry)


def sd_summary(d2map: torch.Tensor, tolerances=(), ranks=()) -> SurfaceSummary:
    """reduces a map of sd_directed_mm on the device; 128 bytes come to the host"""
    import numpy as np
    _need_gpu(d2map)
    assert d2map.dtype == torch.float64 and d2map.is_contiguous()
    tolerances, ranks = [float(t) for t in tolerances], [int(r) for r in ranks]
    scratch = torch.empty(lib().msseg_sd_summary_scratch_bytes(), dtype=torch.uint8, device=d2map.device)
    out = torch.empty(16, dtype=torch.int64, device=d2map.device)
    tol = (C.c_double * max(len(tolerances), 1))(*tolerances)
    rk = (C.c_longlong * max(len(ranks), 1))(*ranks)
    _ck(lib().msseg_sd_summary(_p(d2map), d2map.numel(), tol, len(tolerances), rk, len(ranks), _p(scratch), scratch.numel(),
                               _p(out), _stream()), "sd_summary")
    rec = out.cpu().numpy()
    f = rec.view(np.float64)
    return SurfaceSummary(int(rec[0]), int(rec[1]), float(f[2]), rec[3:3 + len(tolerances)].copy(),
                          f[11:11 + len(ranks)].copy())


def keep_largest_u8(lab: torch.Tensor, n_classes: int, connectivity: int = 26, out: Optional[torch.Tensor] = None,
                    return_stats: bool = False):
    """uint8 [D, H, W] label map -> the map with only the largest connected component of every class 1..n_classes-1
    (MONAI KeepLargestConnectedComponent, independent; connectivity 6 or 26; ties: first voxel in flat order); class 0 and
    values >= n_classes are copied.  out may be lab (in place).  return_stats: also int32 [n_classes, 4] on the device =
    {components, voxels kept, flat index of the kept component's first voxel (-1: absent), voxels removed}."""
    _need_gpu(lab, out)
    assert lab.dtype == torch.uint8 and lab.is_contiguous() and lab.dim() == 3, \
        "keep_largest_u8: lab must be a contiguous uint8 [D, H, W] tensor"
    if out is None:
        out = torch.empty_like(lab)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == lab.shape, \
        "keep_largest_u8: out must be a contiguous uint8 tensor of lab's shape"
    D, H, W = lab.shape
    work = torch.empty(2, lab.numel(), dtype=torch.int32, device=lab.device)
    stats = torch.empty(max(int(n_classes), 1), 4, dtype=torch.int32, device=lab.device)
    _ck(lib().msseg_keep_largest_u8(_p(lab), D, H, W, int(n_classes), int(connectivity), _p(work), _p(stats), _p(out),
                                    _stream()), "keep_largest_u8")
    return (out, stats) if return_stats else out


def postprocess_u8(lab: torch.Tensor, n_classes: int, min_size: int = 0, keep_largest: bool = False, connectivity: int = 26,
                   fill_holes: bool = False, hole_connectivity: int = 26, out: Optional[torch.Tensor] = None,
                   return_stats: bool = False):
    """uint8 [D, H, W] label map -> the map after up to three steps, in this order: components of a class 1..n_classes-1
    with fewer than min_size voxels become 0 (0, 1: off); only the largest component of every class stays (keep_largest,
    keep_largest_u8's rule; both steps label with `connectivity`); holes of class 1, 2, .. are filled in that order
    (fill_holes: scipy binary_fill_holes per class, `hole_connectivity` is that of the leak path).  With all steps off: a
    copy.  out may be lab (in place).  return_stats: also int32 [n_classes, 6] on the device = {components before any step
    (-1 when neither of the first two steps is on), components removed as small, voxels removed as small, voxels removed
    by keep-largest, voxels filled, voxels of the class in the result}."""
    _need_gpu(lab, out)
    assert lab.dtype == torch.uint8 and lab.is_contiguous() and lab.dim() == 3, \
        "postprocess_u8: lab must be a contiguous uint8 [D, H, W] tensor"
    if out is None:
        out = torch.empty_like(lab)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == lab.shape, \
        "postprocess_u8: out must be a contiguous uint8 tensor of lab's shape"
    D, H, W = lab.shape
    work = torch.empty(2, lab.numel(), dtype=torch.int32, device=lab.device)
    stats = torch.empty(max(int(n_classes), 1), 6, dtype=torch.int32, device=lab.device)
    _ck(lib().msseg_postprocess_u8(_p(lab), D, H, W, int(n_classes), int(min_size), int(bool(keep_largest)), int(connectivity),
                                   int(bool(fill_holes)), int(hole_connectivity), _p(work), _p(stats), _p(out), _stream()),
        "postprocess_u8")
    return (out, stats) if return_stats else out


def aug_crop_batch(img, lab, table, out_img, out_lab, roi):
    """img fp32 [C, D, H, W]; lab uint8 [D, H, W] or None; table: uint8 device tensor of npatch msseg_aug_row structs"""
    _need_gpu(img, table, out_img)
    assert img.dtype == torch.float32 and img.is_contiguous() and out_img.is_contiguous()
    npatch = out_img.shape[0]
    assert table.numel() >= npatch * 32
    _ck(lib().msseg_aug_crop_batch(_p(img), _p(lab), img.shape[0], img.shape[1], img.shape[2], img.shape[3], _p(table),
                                   npatch, _p(out_img), dt(out_img), _p(out_lab), roi, _stream()), "aug_crop_batch")
    return out_img, out_lab


# --------------------------------------------------------------------------------------------
# Dataset path (csrc/dataprep.hip): one-off preprocessing of a volume and the multi-volume patch gather
# --------------------------------------------------------------------------------------------
INTENSITY_NONE, INTENSITY_RANGE, INTENSITY_CUBED = 0, 1, 2


def intensity_prep(src, mode=INTENSITY_NONE, a_min=0.0, a_max=1.0, normalize=None):
    """src fp32 / int16 [C, D, H, W] -> (fp32 [C, D, H, W], box int32 [6] on the device: min z, y, x, max z, y, x inclusive
    of the voxels > 0 after scaling, {D, H, W, -1, -1, -1} when none).  normalize: None or (subtrahend, divisor).
    INTENSITY_CUBED takes the cube roots of the bounds on the host (np.cbrt in double, as the reference's transform)."""
    import numpy as np
    _need_gpu(src)
    assert src.dim() == 4 and src.is_contiguous() and src.dtype in (torch.float32, torch.int16)
    if mode == INTENSITY_CUBED:
        a_min, a_max = float(np.cbrt(float(a_min))), float(np.cbrt(float(a_max)))
    dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    box = torch.empty(6, dtype=torch.int32, device=src.device)
    sub, div = (float(normalize[0]), float(normalize[1])) if normalize is not None else (0.0, 1.0)
    _ck(lib().msseg_intensity_prep(_p(src), 0 if src.dtype == torch.float32 else 1, *src.shape, int(mode), float(a_min),
                                   float(a_max) - float(a_min), int(normalize is not None), sub, div, _p(dst), _p(box),
                                   _stream()), "intensity_prep")
    return dst, box


def resample_spacing(src, out_size, ratio):
    """Spacingd: src fp32 (trilinear, border clamp) or uint8 (nearest) [C, D, H, W] -> [C, *out_size]; ratio = new / old
    spacing per axis (source coordinate = destination index * ratio)"""
    _need_gpu(src)
    assert src.dim() == 4 and src.is_contiguous() and src.dtype in (torch.float32, torch.uint8)
    td, th, tw = (int(v) for v in out_size)
    dst = torch.empty(src.shape[0], td, th, tw, dtype=src.dtype, device=src.device)
    _ck(lib().msseg_resample_spacing(_p(src), int(src.dtype == torch.uint8), *src.shape, _p(dst), td, th, tw,
                                     float(ratio[0]), float(ratio[1]), float(ratio[2]), _stream()), "resample_spacing")
    return dst


def crop_pad_copy(src, box, min_size=None, pad_value=0):
    """src fp32 / uint8 [C, D, H, W]; box = (z0, y0, x0, z1, y1, x1) half-open -> the box, padded with pad_value up to
    min_size per axis (MONAI SpatialPad split: (target - n) // 2 before, the rest after).  -> (tensor, pad_before)"""
    _need_gpu(src)
    assert src.dim() == 4 and src.is_contiguous() and src.dtype in (torch.float32, torch.uint8)
    box = [int(v) for v in box]
    n = [box[3 + a] - box[a] for a in range(3)]
    tgt = [max(n[a], int(min_size[a])) if min_size is not None else n[a] for a in range(3)]
    before = [(tgt[a] - n[a]) // 2 for a in range(3)]
    dst = torch.empty(src.shape[0], *tgt, dtype=src.dtype, device=src.device)
    _ck(lib().msseg_crop_pad_copy(_p(src), src.element_size(), *src.shape, (C.c_int * 6)(*box), _p(dst), *tgt,
                                  (C.c_int * 3)(*before), float(pad_value), int(pad_value) if src.dtype == torch.uint8 else 0,
                                  _stream()), "crop_pad_copy")
    return dst, tuple(before)


BG_RULES = {"gt": 0, "ne": 1}


def _bg_rule(rule):
    if rule not in BG_RULES:
        raise ValueError(f"background rule {rule!r}: 'gt' (image > threshold) or 'ne' (image != threshold)")
    return BG_RULES[rule]


def _check_volume(img, lab):
    _need_gpu(img, lab)
    assert img.dtype == torch.float32 and lab.dtype == torch.uint8 and img.is_contiguous() and lab.is_contiguous()
    assert img.dim() == 4 and lab.dim() == 3 and img.shape[1:] == lab.shape


def _check_pick_tables(volumes, nvol, rows, nrows, out):
    """the device tables of the pick calls: nvol msseg_volume_desc, nrows msseg_pick_row, int32 out [nrows, 8]"""
    assert volumes.numel() >= nvol * 32 and rows.numel() >= nrows * 32 and out.dtype == torch.int32
    assert out.is_contiguous() and out.numel() >= nrows * 8


def slab_counts(img, lab, threshold=0.0, rule="gt"):
    """img fp32 [C, D, H, W] (channel 0 is read), lab uint8 [D, H, W] -> int32 [D, 2] on the device:
    per z-slice #(lab > 0), #(lab == 0 and img[0] > threshold); rule "ne": img[0] != threshold, the non-zero mask of a
    z-scored cache"""
    _check_volume(img, lab)
    out = torch.empty(lab.shape[0], 2, dtype=torch.int32, device=lab.device)
    _ck(lib().msseg_slab_counts(_p(img), _p(lab), *lab.shape, float(threshold), _bg_rule(rule), _p(out), _stream()),
        "slab_counts")
    return out


def pick_voxels(volumes, nvol, rows, nrows, roi, threshold, out, rule="gt"):
    """volumes: uint8 device tensor of nvol msseg_volume_desc; rows: uint8 device tensor of nrows msseg_pick_row;
    out: int32 [nrows, 8] on the device; rule as slab_counts"""
    _need_gpu(volumes, rows, out)
    _check_pick_tables(volumes, nvol, rows, nrows, out)
    _ck(lib().msseg_pick_voxels(_p(volumes), nvol, _p(rows), nrows, int(roi), float(threshold), _bg_rule(rule), _p(out),
                                _stream()), "pick_voxels")
    return out


# ---- class-ratio crop centres (csrc/class_crop.hip) --------------------------------------------------------------------
PICK_CLASS0 = 16            # MSSEG_PICK_CLASS0: a pick row of class c carries mode PICK_CLASS0 + c
MAX_CROP_CLASSES = 16
MAX_CENTER_DILATION = 254


def class_candidate_mask(img, lab, classes, dilation, threshold=0.0, rule="gt"):
    """img fp32 [C, D, H, W] (channel 0 is read), lab uint8 [D, H, W], classes: the class numbers (each in 0..15) to build
    -> uint16 [D, H, W] on the device: bit c is set where image_ok(img[0]) (rule as slab_counts) and a voxel of label c lies
    within L1 distance `dilation` (0..254); bits of other classes are 0.  One byte per voxel of scratch for the call."""
    _check_volume(img, lab)
    n = int(dilation)
    if not 0 <= n <= MAX_CENTER_DILATION:
        raise ValueError(f"centre dilation {dilation!r}: 0..{MAX_CENTER_DILATION} (the chamfer distances are bytes)")
    bits = 0
    for c in classes:
        if not 0 <= int(c) < MAX_CROP_CLASSES:
            raise ValueError(f"class {c!r}: 0..{MAX_CROP_CLASSES - 1}")
        bits |= 1 << int(c)
    mask = torch.empty(lab.shape, dtype=torch.uint16, device=lab.device)
    scratch = torch.empty(lab.shape, dtype=torch.uint8, device=lab.device)
    _ck(lib().msseg_class_candidate_mask(_p(img), _p(lab), *lab.shape, float(threshold), _bg_rule(rule), bits, n, _p(scratch),
                                         _p(mask), _stream()), "class_candidate_mask")
    return mask


def class_slab_counts(img, lab, n_classes, threshold=0.0, rule="gt", mask=None):
    """-> int32 [D, n_classes] on the device: per z-slice the candidates of every class c < n_classes (<= 16), i.e.
    #(lab == c and image_ok(img[0])), or, with a class_candidate_mask(...) `mask`, #(bit c of mask)"""
    _check_volume(img, lab)
    K = int(n_classes)
    if not 1 <= K <= MAX_CROP_CLASSES:
        raise ValueError(f"{n_classes!r} classes: 1..{MAX_CROP_CLASSES}")
    if mask is not None:
        _need_gpu(mask)
        assert mask.dtype == torch.uint16 and mask.is_contiguous() and mask.shape == lab.shape
    out = torch.empty(lab.shape[0], K, dtype=torch.int32, device=lab.device)
    _ck(lib().msseg_class_slab_counts(_p(img), _p(lab), _p(mask), *lab.shape, K, float(threshold), _bg_rule(rule), _p(out),
                                      _stream()), "class_slab_counts")
    return out


def class_pick_voxels(volumes, nvol, rows, nrows, roi, threshold, out, rule="gt", masks=None):
    """pick_voxels whose rows may carry mode PICK_CLASS0 + c: the rank-th candidate of class c of the row's slice.  masks:
    None, or an int64 device tensor of nvol pointers to the volumes' candidate masks (0: that volume has none; its class
    rows then read the label)"""
    _need_gpu(volumes, rows, out, masks)
    _check_pick_tables(volumes, nvol, rows, nrows, out)
    if masks is not None:
        assert masks.dtype == torch.int64 and masks.is_contiguous() and masks.numel() >= nvol
    _ck(lib().msseg_class_pick_voxels(_p(volumes), _p(masks), nvol, _p(rows), nrows, int(roi), float(threshold),
                                      _bg_rule(rule), _p(out), _stream()), "class_pick_voxels")
    return out


# ---- per-volume z-score over the non-zero voxels (csrc/volume_stats.hip) ----------------------------------------------
def _flat_channels(x):
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 2, "a contiguous fp32 [C, ...] tensor expected"
    return int(x.shape[0]), int(x.numel() // x.shape[0])


def _stats_scratch(x):
    return torch.empty(lib().msseg_volume_stats_scratch_bytes(int(x.shape[0])), dtype=torch.uint8, device=x.device)


def select_f32(x, ranks=None, percentages=None, scratch=None):
    """exact order statistics of the non-zero values of every channel of x fp32 [C, ...]: `ranks` (1..4 zero-based ranks) or
    `percentages` (1..2 values in [0, 100]: the ranks k, k + 1 of numpy's linear percentile, formed on the device) ->
    float64 [C, 8] on the device = {n, up to 4 order statistics (NaN: rank >= n), P of each percentage as fp32 (-inf, +inf
    where none is formed), 0}.  Nothing is read back."""
    C_, V = _flat_channels(x)
    assert (ranks is None) != (percentages is None), "select_f32: ranks or percentages"
    scratch = _stats_scratch(x) if scratch is None else scratch
    out = torch.empty(C_, 8, dtype=torch.float64, device=x.device)
    rk = (C.c_longlong * len(ranks))(*[int(r) for r in ranks]) if ranks is not None else None
    pc = (C.c_double * len(percentages))(*[float(q) for q in percentages]) if percentages is not None else None
    _ck(lib().msseg_select_f32(_p(x), C_, V, rk, len(ranks) if ranks is not None else 0, pc,
                               len(percentages) if percentages is not None else 0, _p(scratch), scratch.numel(), _p(out),
                               _stream()), "select_f32")
    return out


def masked_moments(x, bounds=None, scratch=None):
    """x fp32 [C, ...]; bounds: None or a float64 [C, 2] device tensor (a view with unit inner stride will do) of clip bounds
    -> float64 [C, 6] on the device = {n, lo, hi, mean, std, number of non-finite masked values} over the non-zero values,
    clipped to [lo, hi] first (tests/zscore_ref.py)"""
    C_, V = _flat_channels(x)
    stride = 0
    if bounds is not None:
        _need_gpu(bounds)
        assert bounds.dtype == torch.float64 and tuple(bounds.shape) == (C_, 2) and bounds.stride(1) == 1
        stride = int(bounds.stride(0)) if C_ > 1 else 2
        assert stride >= 2
    scratch = _stats_scratch(x) if scratch is None else scratch
    stats = torch.empty(C_, 6, dtype=torch.float64, device=x.device)
    _ck(lib().msseg_masked_moments(_p(x), C_, V, _p(bounds), stride, _p(scratch), scratch.numel(), _p(stats), _stream()),
        "masked_moments")
    return stats


def zscore_apply_(x, stats):
    """in place: x = (clip(x, lo, hi) - mean) / std on the non-zero voxels of every channel, with the fp32 values of
    stats (masked_moments' [C, 6])"""
    C_, V = _flat_channels(x)
    _need_gpu(stats)
    assert stats.dtype == torch.float64 and stats.is_contiguous() and tuple(stats.shape) == (C_, 6)
    _ck(lib().msseg_zscore_apply(_p(x), C_, V, _p(stats), _stream()), "zscore_apply")
    return x


def zscore_nonzero_(img, clip=None):
    """--t_zscore on one cached volume, in place: every channel of img fp32 [C, D, H, W] normalised by the mean and the
    population std of its own non-zero voxels; clip = (LO, HI) percentages: those voxels are first clipped to the channel's
    own percentiles.  -> stats, float64 [C, 6] on the device = {n, P_LO, P_HI, mean, std, non-finite count} (bounds -inf,
    +inf without clip).  The whole sequence is enqueued without a host synchronisation."""
    scratch = _stats_scratch(img)
    bounds = None
    if clip is not None:
        lo, hi = clip
        bounds = select_f32(img, percentages=(lo, hi), scratch=scratch)[:, 5:7]
    stats = masked_moments(img, bounds, scratch=scratch)
    zscore_apply_(img, stats)
    return stats


def _check_crop_tables(volumes, nvol, rows, picks, out_img, out_lab, roi):
    """the device tables and outputs of the crop gathers; -> the number of patches"""
    npatch = out_img.shape[0]
    assert volumes.numel() >= nvol * 32 and rows.numel() >= npatch * 32 and picks.numel() >= npatch * 8
    assert picks.dtype == torch.int32 and picks.is_contiguous() and out_img.is_contiguous() and out_lab.is_contiguous()
    assert out_lab.dtype == torch.float32 and out_lab.numel() == npatch * roi ** 3 and tuple(out_img.shape[2:]) == (roi,) * 3
    return npatch


def aug_crop_multi(volumes, nvol, rows, picks, out_img, out_lab, roi):
    """one gather launch for a batch over many cached volumes; out_img [n, C, R, R, R] fp32 / bf16, out_lab fp32 [n, 1, R, R, R].
    The descriptor and row tables are device memory: the caller guarantees that every row names one of the nvol volumes,
    that it has out_img's channel count and holds an roi^3 patch (DeviceDatasetLoader checks this at construction); a row
    that does not comes back as an all-zero patch."""
    _need_gpu(volumes, rows, picks, out_img, out_lab)
    npatch = _check_crop_tables(volumes, nvol, rows, picks, out_img, out_lab, roi)
    _ck(lib().msseg_aug_crop_multi(_p(volumes), nvol, _p(rows), _p(picks), npatch, out_img.shape[1], _p(out_img), dt(out_img),
                                   _p(out_lab), int(roi), _stream()), "aug_crop_multi")
    return out_img, out_lab


def aug_crop_affine(volumes, nvol, rows, picks, mats, out_img, out_lab, roi, pad_value=0.0):
    """aug_crop_multi sampling the cached volume under a matrix per patch, in one launch: mats float64 [n, 3, 3] on the
    device (row-major M; source = patch centre + M (patch index - (roi - 1) / 2)), image trilinear with taps outside the
    volume reading pad_value, label nearest with 0 outside.  Identity matrices give aug_crop_multi's output bit for bit.
    Tables and preconditions as aug_crop_multi."""
    _need_gpu(volumes, rows, picks, mats, out_img, out_lab)
    npatch = _check_crop_tables(volumes, nvol, rows, picks, out_img, out_lab, roi)
    assert mats.dtype == torch.float64 and mats.is_contiguous() and mats.numel() == npatch * 9
    _ck(lib().msseg_aug_crop_affine(_p(volumes), nvol, _p(rows), _p(picks), _p(mats), npatch, out_img.shape[1], _p(out_img),
                                    dt(out_img), _p(out_lab), int(roi), float(pad_value), _stream()), "aug_crop_affine")
    return out_img, out_lab


INTENSITY_NOISE, INTENSITY_BLUR, INTENSITY_CONTRAST, INTENSITY_GAMMA_INV, INTENSITY_GAMMA = 1, 2, 4, 8, 16
INTENSITY_ROW_BYTES = 32


def intensity_aug(batch_f32, table, out_dtype=torch.float32, out=None):
    """noise -> blur -> contrast -> gamma on the inverted image -> gamma on a gathered batch (csrc/intensity_aug.hip).
    batch_f32: contiguous fp32 [N, C, D, H, W] on the GPU; table: the N * C rows msseg_intensity_row (row n * C + c) as a
    sequence or array of data_device.IntensityRow on the HOST -- the entry point validates and plans from them; they are
    uploaded here for the kernels.  -> the batch in out_dtype (fp32 / bf16), written into `out` when given.  Refused with
    nothing launched: a CPU tensor, another dtype, a non-contiguous batch, a patch dimension below 8, a blur sigma above 2."""
    _need_gpu(batch_f32, out)
    if batch_f32.dtype != torch.float32:
        raise TypeError(f"intensity_aug takes a float32 batch, got {batch_f32.dtype}")
    if out_dtype not in _DT:
        raise TypeError(f"unsupported dtype {out_dtype} (float32 / bfloat16 only)")
    if batch_f32.dim() != 5 or not batch_f32.is_contiguous():
        raise ValueError("intensity_aug takes a contiguous [N, C, D, H, W] batch")
    N, Cc, D, H, W = batch_f32.shape
    raw = bytes(table) if isinstance(table, (C.Array, bytes, bytearray)) else b"".join(bytes(r) for r in table)
    if len(raw) != N * Cc * INTENSITY_ROW_BYTES:
        raise ValueError(f"intensity_aug: {N} x {Cc} patches and channels need {N * Cc} rows of {INTENSITY_ROW_BYTES} bytes, "
                         f"got {len(raw)} bytes")
    if out is None:
        out = torch.empty(batch_f32.shape, dtype=out_dtype, device=batch_f32.device)
    elif out.dtype != out_dtype or out.shape != batch_f32.shape or not out.is_contiguous() or out.device != batch_f32.device:
        raise ValueError("intensity_aug: out must be a contiguous tensor of the batch's shape and device in out_dtype")
    host = C.create_string_buffer(raw, len(raw))
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(batch_f32.device)   # blocking: the host copy may go
    ws, ws_bytes = None, 0
    if any(raw[j] & (INTENSITY_CONTRAST | INTENSITY_GAMMA_INV | INTENSITY_GAMMA) for j in range(0, len(raw), INTENSITY_ROW_BYTES)):
        ws_bytes = int(lib().msseg_intensity_aug_workspace_bytes(N, Cc, D, H, W))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=batch_f32.device)
    _ck(lib().msseg_intensity_aug(_p(batch_f32), C.cast(host, C.c_void_p), _p(dev), N, Cc, D, H, W, _p(out), _DT[out_dtype],
                                  _p(ws) if ws is not None else None, ws_bytes, _stream()), "intensity_aug")
    return out


def intensity_noise_bits(key, n, first=0, device="cuda"):
    """the four Philox4x32-10 words of counters first .. first + n - 1 under the 64-bit key, as int32 [n, 4] (bit patterns of
    the uint32 words): the integer stage of intensity_aug's noise, for comparison with its numpy restatement"""
    out = torch.empty(int(n), 4, dtype=torch.int32, device=device)
    _need_gpu(out)
    _ck(lib().msseg_intensity_noise_bits(int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF, int(first), int(n), _p(out), _stream()), "intensity_noise_bits")
    return out


# --------------------------------------------------------------------------------------------
# Swin pieces
# --------------------------------------------------------------------------------------------
def conv3d_k3s2(x, wp, bias, y, cin, cout):
    _need_gpu(x, wp, y)
    N, D, H, W = x.shape[:4]
    _ck(lib().msseg_conv3d_k3s2_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(y), ld(y), N, D, H, W, cin, cout, dt(x),
                                    _stream()), "conv3d_k3s2_fwd")
    return y


def box_copy(src, dst):
    """dst[n, d, h, w, :] = src[n, d, h, w, :] inside the common box, zero elsewhere in dst (channels-last [N, D, H, W, C]): zero
    padding at the high end of the spatial axes, or the crop back -- each is the other's adjoint (csrc/layout.hip)"""
    _need_gpu(src, dst)
    N, SD, SH, SW, Cc = src.shape
    _, DD, DH, DW, Cd = dst.shape
    if Cc != Cd or dst.shape[0] != N or src.dtype != dst.dtype:
        raise ValueError("box_copy: batch, channel count and dtype must agree")
    _ck(lib().msseg_box_copy(_p(src), ld(src), SD, SH, SW, _p(dst), ld(dst), DD, DH, DW, N, Cc, dt(src), _stream()), "box_copy")
    return dst


def merge_subs(offsets) -> int:
    """eight (a, b, c) sub-grid offsets along (D, H, W) -> the packed `subs` word of merge_gather"""
    assert len(offsets) == 8
    word = 0
    for s, (a, b, c) in enumerate(offsets):
        word |= (a | (b << 1) | (c << 2)) << (3 * s)
    return word


def merge_gather(x, out, subs):
    """out[n, i, j, k, s*C + c] = x[n, 2i + a_s, 2j + b_s, 2k + c_s, c] (zero beyond the grid): PatchMerging's eight strided
    slices + concat in one pass"""
    _need_gpu(x, out)
    N, D, H, W, Cc = x.shape
    _ck(lib().msseg_merge_gather_fwd(_p(x), ld(x), D, H, W, _p(out), ld(out), N, Cc, subs, dt(x), _stream()), "merge_gather_fwd")
    return out


def merge_gather_bwd(dy, dx, subs):
    """adjoint of merge_gather: dx [N, D, H, W, C] from dy [N, ceil(D/2), ceil(H/2), ceil(W/2), 8C]"""
    _need_gpu(dy, dx)
    N, D, H, W, Cc = dx.shape
    _ck(lib().msseg_merge_gather_bwd(_p(dy), ld(dy), _p(dx), ld(dx), N, D, H, W, Cc, subs, dt(dx), _stream()), "merge_gather_bwd")
    return dx


def zero_stuff2(dy, out):
    """dy [N,OD,OH,OW,C] -> out [N,ID,IH,IW,C] with out[:, ::2, ::2, ::2] = dy and zeros elsewhere."""
    _need_gpu(dy, out)
    N, OD, OH, OW, Cc = dy.shape
    ID, IH, IW = out.shape[1:4]
    _ck(lib().msseg_zero_stuff2(_p(dy), ld(dy), _p(out), ld(out), N, OD, OH, OW, ID, IH, IW, Cc, dt(dy), _stream()),
        "zero_stuff2")
    return out


def _attn_table_stride(table, B, heads, bws):
    """0 for a shared bias table [M3, heads]; M3 * heads for per-sample tables [B, M3, heads] fp32 contiguous"""
    if table.dim() != 3:
        return 0
    assert table.is_contiguous() and table.dtype == torch.float32
    assert table.shape == (B, (2 * bws - 1) ** 3, heads), table.shape
    return table[0].numel()


def window_attention_fwd(qkv, qkv_bias, table, out, heads, ws, shift, bias_ws=None):
    """qkv [B,S,H,W,3C] contiguous -> out [B,S,H,W,C]; returns lse for the backward.  table: [M3, heads] shared by every
    sample, or [B, M3, heads] with one table per sample.  bias_ws: window edge the bias table was built for (MONAI
    SwinUNETR: 7 even where the window is clamped to a smaller grid)."""
    _need_gpu(qkv, table, out)
    assert qkv.is_contiguous() and out.is_contiguous()
    B, S, H, W, C3 = qkv.shape
    bws = bias_ws or ws
    nW = -(-S // ws) * -(-H // ws) * -(-W // ws)
    lse = torch.empty(B * nW, heads, ws ** 3, dtype=torch.float32, device=qkv.device)
    _ck(lib().msseg_window_attention_fwd(_p(qkv), _p(qkv_bias), _p(table), _p(out), _p(lse), B, S, H, W, C3 // 3, heads, ws,
                                         shift, bws, _attn_table_stride(table, B, heads, bws), dt(qkv), _stream()),
        "window_attention_fwd")
    return lse


def window_attention_bwd(qkv, qkv_bias, table, out, lse, dout, dqkv, dtable, heads, ws, shift, bias_ws=None):
    """backward of window_attention_fwd; dtable (nullable, shaped like table) is ACCUMULATED, per sample for per-sample
    tables"""
    _need_gpu(qkv, table, out, lse, dout, dqkv)
    assert qkv.is_contiguous() and out.is_contiguous() and dout.is_contiguous() and dqkv.is_contiguous()
    B, S, H, W, C3 = qkv.shape
    bws = bias_ws or ws
    stride = _attn_table_stride(table, B, heads, bws)
    wsb = 0
    if dtable is not None:
        assert stride == 0 or (dtable.is_contiguous() and dtable.shape == table.shape)
        wsb = int(lib().msseg_window_attention_bwd_workspace_bytes(B, S, H, W, C3 // 3, heads, ws, shift, bws, stride,
                                                                    dt(qkv)))
    work = torch.empty(wsb, dtype=torch.uint8, device=qkv.device) if wsb else None
    _ck(lib().msseg_window_attention_bwd(_p(qkv), _p(qkv_bias), _p(table), _p(out), _p(lse), _p(dout), _p(dqkv),
                                         _p(dtable), B, S, H, W, C3 // 3, heads, ws, shift, bws, stride, dt(qkv), _p(work),
                                         wsb, _stream()), "window_attention_bwd")
    return dqkv


AFFINE_ACC_TABLE, AFFINE_ACC_EMB, AFFINE_ACC_LIN_W, AFFINE_ACC_LIN_B = 1, 2, 4, 8


def rel_bias_affine_fold(table, emb, lin_w, lin_b, aff, out):
    """out [B, M3, heads] = table + lin_b + sum_k lin_w[k] * aff[b, k] * emb[..., k]  (all fp32, contiguous, on the GPU)"""
    _need_gpu(table, emb, lin_w, lin_b, aff, out)
    M3, heads = table.shape
    B = aff.shape[0]
    assert emb.shape == (M3, heads, 3) and lin_w.numel() == 3 and lin_b.numel() == 1 and aff.shape == (B, 3)
    assert out.shape == (B, M3, heads)
    for t in (table, emb, lin_w, lin_b, aff, out):
        assert t.dtype == torch.float32 and t.is_contiguous()
    _ck(lib().msseg_rel_bias_affine_fold(_p(table), _p(emb), _p(lin_w), _p(lin_b), _p(aff), _p(out), B, M3, heads,
                                         _stream()), "rel_bias_affine_fold")
    return out


def rel_bias_affine_grad(dT, emb, lin_w, aff, dtable=None, demb=None, dlin_w=None, dlin_b=None, flags=0):
    """parameter gradients from the per-sample table gradient dT [B, M3, heads]; each output (nullable) is overwritten, or
    accumulated when its AFFINE_ACC_* bit is in `flags`"""
    _need_gpu(dT, emb, lin_w, aff)
    B, M3, heads = dT.shape
    for t in (dT, emb, lin_w, aff, dtable, demb, dlin_w, dlin_b):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda)
    assert emb.shape == (M3, heads, 3) and aff.shape == (B, 3)
    assert dtable is None or dtable.numel() == M3 * heads
    assert demb is None or demb.numel() == M3 * heads * 3
    assert (dlin_w is None or dlin_w.numel() == 3) and (dlin_b is None or dlin_b.numel() == 1)
    wsb = int(lib().msseg_rel_bias_affine_grad_workspace_bytes(M3, heads))
    work = torch.empty(wsb, dtype=torch.uint8, device=dT.device)
    _ck(lib().msseg_rel_bias_affine_grad(_p(dT), _p(emb), _p(lin_w), _p(aff), _p(dtable), _p(demb), _p(dlin_w),
                                         _p(dlin_b), B, M3, heads, int(flags), _p(work), wsb, _stream()),
        "rel_bias_affine_grad")


def layernorm_fwd(x, gamma, beta, y, eps=1e-5, save=True):
    _need_gpu(x, y)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save else None
    _ck(lib().msseg_layernorm_fwd(_p(x), ld(x), _p(gamma), _p(beta), _p(y), ld(y), _p(mean), _p(rstd), rows, Cc, eps,
                                  dt(x), _stream()), "layernorm_fwd")
    return mean, rstd


def layernorm_bwd_add_ok(x) -> bool:
    """does layernorm_bwd(..., add=) take rows shaped like x's (the vector kernel: 16-byte chunks, at most 4096 channels)?"""
    epc = 16 // x.element_size()
    return x.shape[-1] % epc == 0 and x.shape[-1] <= 512 * epc and x.data_ptr() % 16 == 0


def layernorm_bwd(x, gamma, mean, rstd, dy, dx, dgamma=None, dbeta=None, accumulate=False, add=None):
    """add (optional, shaped like x): dx = layernorm backward + add in the same pass (layernorm_bwd_add_ok(x))"""
    _need_gpu(x, dy, dx)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    if add is not None:
        _ck(lib().msseg_layernorm_bwd_add(_p(x), ld(x), _p(gamma), _p(mean), _p(rstd), _p(dy), ld(dy), _p(add), ld(add), _p(dx),
                                          ld(dx), rows, Cc, dt(x), _stream()), "layernorm_bwd_add")
    else:
        _ck(lib().msseg_layernorm_bwd(_p(x), ld(x), _p(gamma), _p(mean), _p(rstd), _p(dy), ld(dy), _p(dx), ld(dx),
                                      rows, Cc, dt(x), _stream()), "layernorm_bwd")
    if dgamma is not None:
        sc = scratch(x.device)
        _ck(lib().msseg_layernorm_param_grad(_p(x), ld(x), _p(mean), _p(rstd), _p(dy), ld(dy), _p(dgamma), _p(dbeta),
                                             int(accumulate),
                                             rows, Cc, _p(sc), sc.numel(), dt(x), _stream()), "layernorm_param_grad")
    return dx


def gelu_fwd(x, y):
    _need_gpu(x, y)
    assert x.is_contiguous() and y.is_contiguous()
    _ck(lib().msseg_gelu_fwd(_p(x), _p(y), x.numel(), dt(x), _stream()), "gelu_fwd")
    return y


def linear_gelu_ok(x, cin, cout) -> bool:
    """fc1 + GELU (and fc2's input gradient + GELU backward) of a cin -> cout MLP on x's tokens run as one launch each"""
    return bool(x.is_cuda and x.dtype == torch.bfloat16 and
                lib().msseg_linear_gelu_ok(x.numel() // x.shape[-1], cin, cout, BF16))


def linear_gelu_fwd(x, wp, bias, pre, act, cin, cout):
    """pre = x W^T + b, act = gelu(pre) in one launch (bit-identical to conv3d_k1 + gelu_fwd)"""
    _need_gpu(x, wp, pre, act)
    nv = x.numel() // x.shape[-1]
    esz = x.element_size()
    TIMER.launch("linear_gelu_fwd", 2.0 * nv * cin * cout, nv * (cin + 2 * cout) * esz + cin * cout * esz,
                 lambda: _ck(lib().msseg_linear_gelu_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(pre), ld(pre), _p(act), ld(act), nv,
                                                         cin, cout, dt(x), _stream()), "linear_gelu_fwd"))
    return pre, act


def linear_gelu_bwd(dy, wp, pre, dpre, cin, cout):
    """dpre = (dy W) * gelu'(pre): cin = channels of dy, cout = channels of pre / dpre (bit-identical to conv3d_k1 + gelu_bwd)"""
    _need_gpu(dy, wp, pre, dpre)
    nv = dy.numel() // dy.shape[-1]
    esz = dy.element_size()
    TIMER.launch("linear_gelu_bwd", 2.0 * nv * cin * cout, nv * (cin + 2 * cout) * esz + cin * cout * esz,
                 lambda: _ck(lib().msseg_linear_gelu_bwd(_p(dy), ld(dy), _p(wp), _p(pre), ld(pre), _p(dpre), ld(dpre), nv, cin,
                                                         cout, dt(dy), _stream()), "linear_gelu_bwd"))
    return dpre


def linear_add_ok(x, res, cin, cout) -> bool:
    """can y = res + Linear(x) run as one launch (bf16, shapes of the register-resident-weight kernel, aligned operands)?"""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and res.dtype == x.dtype and x.data_ptr() % 16 == 0 and res.data_ptr() % 16 == 0):
        return False
    return bool(lib().msseg_linear_add_ok(x.numel() // x.shape[-1], cin, cout, BF16))


def linear_add(x, wp, bias, res, y, cin, cout):
    """y = res + (x W^T + b) (the bf16-rounded Linear output added to res: bit-identical to conv3d_k1 followed by an add pass)"""
    _need_gpu(x, wp, res, y)
    nv = x.numel() // x.shape[-1]
    esz = x.element_size()
    TIMER.launch("linear_add_fwd", 2.0 * nv * cin * cout, nv * (cin + 2 * cout) * esz + cin * cout * esz,
                 lambda: _ck(lib().msseg_linear_add_fwd(_p(x), ld(x), _p(wp), _p(bias), _p(res), ld(res), _p(y), ld(y), nv, cin, cout,
                                                        dt(x), _stream()), "linear_add_fwd"))
    return y


def gelu_bwd(x, dy, dx):
    _need_gpu(x, dy, dx)
    assert x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous()
    _ck(lib().msseg_gelu_bwd(_p(x), _p(dy), _p(dx), x.numel(), dt(x), _stream()), "gelu_bwd")
    return dx
