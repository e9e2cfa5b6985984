"""CLI of the training / evaluation drivers: every flag of ``/root/reference/utils/arguments.py:29-313`` with
the same name, type, default and list-collapsing rule (``:19-24``: a list argument of length 1 becomes a scalar,
longer lists become tuples), declared as a table; plus a few flags of this build (synthetic data, compute
dtype, hipGraph replay, post-processing, rotation + zoom in the device crop gather, mirror test-time augmentation, intensity augmentation, per-volume z-score, class-ratio crop centres, file inference).  Flags whose subsystem is out of the hot-path scope (learned class vectors, MONAI
transforms, Neptune) are accepted and ignored so reference command lines keep working."""
from __future__ import annotations

import argparse

S, I, F = str, int, float
# (flag, kind, default, type)   kind: v = value, l = list (nargs='*'), t = store_true, f = store_false(dest),
#                               c = value out of the choices in a fifth field
_SPEC = {
    "model": [
        ("--model", "v", "UNETR_Official", S), ("--vol_size", "l", [96], I), ("--patch_size", "l", [16], I),
        ("--window_size", "l", [6], I), ("--input_dim", "v", 3, I), ("--output_dim", "v", 3, I),
        ("--in_chans", "v", 1, I), ("--hidden_dim", "v", 48, I), ("--depths", "l", [2, 2, 2, 2], I),
        ("--num_heads", "l", [3, 6, 12, 24], I), ("--mlp_ratio", "v", 4.0, F), ("--rel_pos_bias", "t"),
        ("--rel_pos_bias_affine", "t"), ("--abs_pos_emb", "t"), ("--rel_crop_pos_emb", "t"), ("--qkv_bias", "t"),
        ("--gradient_clipping", "v", None, F), ("--mixed_precision", "t"), ("--learned_cls_vectors", "t"),
        ("--lcv_vector_dim", "v", 6, I), ("--lcv_final_layer", "t"), ("--lcv_sincos_emb", "t"),
        ("--lcv_concat_vector", "t"), ("--lcv_only", "t"), ("--lcv_linear_comb", "t"), ("--lcv_patch_voxel_mean", "t"),
        ("--use_abs_pos_emb", "t"), ("--global_token", "t"),
    ],
    "transform": [
        ("--t_voxel_spacings", "t"), ("--t_voxel_dims", "l", [1.0], F), ("--t_cubed_ct_intensity", "t"),
        ("--t_fixed_ct_intensity", "t"), ("--t_percentile_ct_intensity", "t"), ("--t_ct_min", "v", -1000, I),
        ("--t_ct_max", "v", 1000, I), ("--t_crop_foreground_img", "t"), ("--t_crop_foreground_kdiv", "t"),
        ("--t_rand_crop_fgbg", "t"), ("--t_rand_crop_pos_weight", "v", 1.0, F), ("--t_rand_crop_neg_weight", "v", 1.0, F),
        ("--t_rand_crop_classes", "t"), ("--t_rand_crop_dilated_center", "t"), ("--t_rand_spatial_crop", "t"),
        ("--t_spatial_pad", "t"), ("--t_convert_labels_to_brats", "t"), ("--t_normalize", "t"),
        ("--t_normalize_channel_wise", "t"), ("--t_norm_mean", "v", 0.1943, F), ("--t_norm_std", "v", 0.2786, F),
        ("--t_n_patches_per_image", "v", 1, I), ("--t_flip_prob", "v", 0.0, F), ("--t_rot_prob", "v", 0.0, F),
        ("--t_intensity_shift_os", "v", 0.1, F), ("--t_intensity_shift_prob", "v", 0.0, F),
        ("--t_intensity_scale_factors", "v", 0.1, F), ("--t_intensity_scale_prob", "v", 0.0, F),
    ],
    "data": [
        ("--data_path", "v", "/datasets/", S), ("--json_list", "v", "dataset.json", S), ("--task", "v", "Task03_Liver", S),
        ("--batch_size_val", "v", 1, I), ("--n_images_per_batch", "v", 8, I), ("--n_workers_train", "v", 8, I),
        ("--n_workers_val", "v", 2, I), ("--no_pin_memory", "f", "pin_mem"), ("--no_cache_dataset", "f", "cache_dataset"),
        ("--cache_rate_train", "v", 1.0, F), ("--cache_rate_val", "v", 1.0, F),
    ],
    "optimizer": [
        ("--loss_fn", "v", "DiceCE", S), ("--tversky_alpha", "v", 0.5, F), ("--tversky_beta", "v", 0.5, F),
        ("--smooth_nr", "v", 1e-5, F), ("--smooth_dr", "v", 1e-5, F), ("--weight_decay", "v", 1e-5, F),
        ("--lr", "v", 4e-4, F), ("--momentum", "v", 0.9, F), ("--warmup_epochs", "v", 40, I),
    ],
    "training": [
        ("--start_epoch", "v", 0, I), ("--epochs", "v", 200, I), ("--save_ckpt_freq", "v", 20, I),
        ("--val_interval", "v", 20, I), ("--cv_fold", "v", 0, I), ("--cv_max_folds", "v", 5, I),
        ("--val_infer_overlap", "v", 0.5, F), ("--world_size", "v", 1, I), ("--local_rank", "v", -1, I),
        ("--dist_on_itp", "t"), ("--dist_url", "v", "env://", S), ("--backend", "v", "nccl", S),
        ("--resume", "v", "", S), ("--pretrained", "v", None, S),
    ],
    "misc": [
        ("--seed", "v", 13, I), ("--no_cuddn_auto_tuner", "t"), ("--anomaly_detection", "t"), ("--log_dir", "v", None, S),
        ("--no_neptune_logging", "f", "neptune_logging"), ("--save_eval_output", "t"), ("--output_dir", "v", None, S),
        ("--description", "v", None, S),
    ],
    "amd": [  # additions of this build
        ("--synthetic", "t"), ("--synthetic_steps", "v", 8, I), ("--synthetic_val_size", "l", [128], I),
        ("--compute_dtype", "v", "bf16", S), ("--flat_optimizer", "t"),
        # post-processing of the predicted label maps (engine/test.py), in this order: drop components below N voxels, keep
        # the largest connected component per class, fill the holes of every class; any of them switches it on
        ("--post_keep_largest", "t"), ("--post_connectivity", "c", 26, I, (6, 26)),
        ("--post_min_size", "v", 0, I), ("--post_fill_holes", "t"), ("--post_hole_connectivity", "c", 26, I, (6, 26)),
        # random rotation + zoom inside the device crop gather (data_device.py): probability per patch, angle bound(s) in
        # degrees (one for all three tensor axes or one per axis, each angle from U(-A, A)), zoom factor from U(LO, HI)
        ("--t_affine_prob", "v", 0.0, F), ("--t_affine_rotate", "l", [30.0], F), ("--t_affine_zoom", "l", [0.7, 1.4], F),
        # mirror test-time augmentation of the sliding-window inference (engine/utils.py): the volume axes (0 = D, 1 = H,
        # 2 = W) to flip; every window is predicted under each of the 2^n flip combinations and the logits are averaged
        ("--infer_mirror_axes", "l", [], I),
        # intensity augmentation of the gathered batch (data_device.py, csrc/intensity_aug.hip), nnU-Net's stages, order and
        # default ranges: a probability per patch and stage, values from U(LO, HI); --t_blur_channel_prob is the share of
        # a chosen patch's channels that are blurred; --t_gamma_range serves both gamma stages
        ("--t_noise_prob", "v", 0.0, F), ("--t_noise_std", "l", [0.0, 0.1], F),
        ("--t_blur_prob", "v", 0.0, F), ("--t_blur_sigma", "l", [0.5, 1.0], F), ("--t_blur_channel_prob", "v", 0.5, F),
        ("--t_contrast_prob", "v", 0.0, F), ("--t_contrast_range", "l", [0.75, 1.25], F),
        ("--t_gamma_invert_prob", "v", 0.0, F), ("--t_gamma_prob", "v", 0.0, F), ("--t_gamma_range", "l", [0.7, 1.5], F),
        # MR data: every channel of every cached volume normalised by the mean and std of its own non-zero voxels, as the
        # last preprocessing step (data_device.py, csrc/volume_stats.hip; nnU-Net's per-volume z-score); --t_zscore_clip
        # LO HI first clips those voxels to the channel's own percentiles, e.g. 0.5 99.5
        ("--t_zscore", "t"), ("--t_zscore_clip", "l", [], F),
        # crop centres per class (data_device.py, csrc/class_crop.hip; the reference's --t_rand_crop_classes is the case NEG
        # POS POS ...): one ratio >= 0 per class, --output_dim of them; a crop flag like --t_rand_crop_fgbg.
        # --t_rand_crop_center_dilation N takes the centres within L1 distance N (0..254) of a class instead of on it (the
        # reference's --t_rand_crop_dilated_center is N = 48)
        ("--t_rand_crop_class_ratios", "l", [], F), ("--t_rand_crop_center_dilation", "v", 0, I),
        # region-based training (nnU-Net): one SIGMOID output per region, a region being a union of label values.  One token
        # SET=VALUE per output channel, --output_dim of them: SET a comma list of label values in 0..31, VALUE the label
        # (0..255) a voxel gets in the decoded map where the region fires, later regions painted over earlier ones.
        # `--output_dim 3 --label_regions 1,2,3=1 2,3=2 3=3` is Decathlon BrainTumour's whole tumour / core / enhancing.
        ("--label_regions", "l", [], S),
    ],
    "file inference": [  # run_predict.py: the files of a data list (engine/test.py, csrc/restore.hip)
        # the section of the data list to predict (labels of "validation" / "training" are ignored)
        ("--test_section", "v", "test", S),
        # how a prediction reaches the file's grid: nearest = the label map is restored; linear = the logits are resampled
        # trilinearly and the arg max is taken per native voxel
        ("--restore_mode", "c", "nearest", S, ("nearest", "linear")),
    ],
}


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="3-D medical segmentation on MI355X")
    for group_name, flags in _SPEC.items():
        g = parser.add_argument_group(group_name)
        for spec in flags:
            flag, kind = spec[0], spec[1]
            if kind == "v":
                g.add_argument(flag, default=spec[2], type=spec[3])
            elif kind == "c":
                g.add_argument(flag, default=spec[2], type=spec[3], choices=spec[4])
            elif kind == "l":
                g.add_argument(flag, nargs="*", default=list(spec[2]), type=spec[3])
            elif kind == "t":
                g.add_argument(flag, action="store_true", default=False)
            else:
                g.add_argument(flag, action="store_false", dest=spec[2], default=True)
    return parser


def collapse_lists(args):
    for k, v in vars(args).items():
        if isinstance(v, list):
            setattr(args, k, v[0] if len(v) == 1 else tuple(v))
    return args


def get_args(argv=None):
    return collapse_lists(build_parser().parse_args(argv))


MAX_REGIONS = 16


def parse_label_regions(tokens, output_dim):
    """``--label_regions`` tokens ``SET=VALUE`` -> ``(masks, values)``: per output channel the uint32 bit mask of the label
    values in its SET (bit l set: label l belongs to the region) and the label VALUE of the decoded map.  A ValueError names
    the flag for: a token count other than ``output_dim``, more than 16 regions, an empty SET, a label outside 0..31, a VALUE
    outside 0..255, a malformed token."""
    flag = "--label_regions"
    if isinstance(tokens, str):
        tokens = [tokens]
    tokens = list(tokens)
    if len(tokens) > MAX_REGIONS:
        raise ValueError(f"{flag}: at most {MAX_REGIONS} regions are supported, got {len(tokens)}")
    if len(tokens) != int(output_dim):
        raise ValueError(f"{flag}: one SET=VALUE token per output channel ({output_dim} for --output_dim {output_dim}), "
                         f"got {len(tokens)}")
    masks, values = [], []
    for tok in tokens:
        head, sep, tail = str(tok).partition("=")
        try:
            if not sep:
                raise ValueError
            labels = [int(v) for v in head.split(",") if v.strip() != ""]
            value = int(tail)
        except ValueError:
            raise ValueError(f"{flag}: `{tok}` is not SET=VALUE with SET a comma list of integers, e.g. 1,2,3=1") from None
        if not labels:
            raise ValueError(f"{flag}: `{tok}` has an empty label set")
        if any(v < 0 or v > 31 for v in labels):
            raise ValueError(f"{flag}: `{tok}` names a label outside 0..31")
        if value < 0 or value > 255:
            raise ValueError(f"{flag}: `{tok}` has a value outside 0..255")
        mask = 0
        for v in labels:
            mask |= 1 << v
        masks.append(mask)
        values.append(value)
    return tuple(masks), tuple(values)


def region_table(cfg):
    """``(masks, values)`` of ``--label_regions`` (parse_label_regions), or None without the flag"""
    tokens = getattr(cfg, "label_regions", None)
    if tokens is None or (not isinstance(tokens, str) and len(tokens) == 0):
        return None
    return parse_label_regions(tokens, cfg.output_dim)


def n_label_values(cfg):
    """number of label values of the label maps: ``--output_dim`` for exclusive classes; under ``--label_regions`` one more
    than the largest label any SET or VALUE names (the output channels are regions then, not label values)"""
    table = region_table(cfg)
    if table is None:
        return cfg.output_dim
    masks, values = table
    return 1 + max(max(m.bit_length() - 1 for m in masks), max(values))
