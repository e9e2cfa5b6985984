"""Evaluation / test-time inference: mirrors ``/root/reference/engine/test.py`` (``eval_model`` :15-94,
``test_model`` :96-173).  The label map is formed on the device (``msseg_argmax_u8``: the arg max of the blended logits,
the reference's softmax is monotonic) and resampled to the original grid with ``msseg_resample_nearest_u8`` (the
reference's ``resample_3d`` = scipy order-0 zoom, ``utils/misc.py:420-425``); only uint8 maps cross PCIe.  Outputs go
to the reference's directory layout as NIfTI-1 files (``utils/nifti.py``: nibabel is not available) when the input names
carry a NIfTI extension, as ``.npy`` otherwise (synthetic loaders).  The Hausdorff-95 meter (``mHdorffDist``, :20,31,48-51,64)
comes from ``metrics.hausdorff95``: surfaces, exact distances and their histogram on the device.

Post-processing of the arg-max maps (an addition of this build, off by default) runs on the device in one call
(``msseg_postprocess_u8``), in this order: ``--post_min_size N`` drops components below N voxels (MONAI
``RemoveSmallObjects``, nnU-Net), ``--post_keep_largest`` keeps the largest component per class (MONAI
``KeepLargestConnectedComponent``; both with ``--post_connectivity`` 6 or 26), ``--post_fill_holes`` fills the holes of
class 1, 2, .. (MONAI ``FillHoles``, ``--post_hole_connectivity`` 6 or 26).  Any of the three switches it on:
``eval_model`` then reports ``ppDice`` and ``ppHdorffDist`` of the processed maps next to the unchanged meters and saves
the processed map; ``test_model`` processes on the model grid, before the resample and before saving; ``run_validation``
(engine/val.py) adds ``ppDice``.

File input (an addition of this build): a batch of ``test_model`` that carries a ``"restore"`` entry (the geometry of its
``data_device.preprocess_volume`` record, ``data_device.restore_geometry``; one record per batch) also gets a map on the
grid of the file it came from, written to ``test_output/Fold<k>/native/<name>`` under the file's full affine (translation
kept; ``pred/``, ``img/`` and ``rs/`` keep the reference's zeroed translation).  ``hip.restore_native_u8`` undoes pad,
foreground crop, spacing resample and RAS reorientation in one launch.  ``--restore_mode nearest`` (default): arg max on
the model grid, post-processing if enabled, then the label map is restored.  ``--restore_mode linear``: the blended logits
are resampled trilinearly and the arg max is taken per native voxel inside the kernel (nnU-Net's order), then
post-processing runs on the native map; ``pred/`` then holds the unprocessed model-grid arg max.  Batches without the entry
behave as before.

Region-based training (``--label_regions``, an addition of this build): the label map is ``hip.region_decode_u8`` of the
sigmoid logits (threshold 0, regions painted in their listed order) instead of the arg max; ``class{c}Dice``, ``ppDice`` and
the Hausdorff meters are per REGION (both maps taken through the region's label set); post-processing runs on the decoded
map over ``n_label_values`` label values.  ``--restore_mode linear`` is refused: the threshold would have to move inside
the restore kernel."""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import hip, metrics
from ..data_device import normalised_zero, output_name
from ..utils import misc
from ..utils.arguments import n_label_values, region_table
from .train import _metric_update
from .utils import sliding_window_inference


def label_map(outputs: torch.Tensor, regions=None) -> torch.Tensor:
    """logits [1, C, D, H, W] -> uint8 [D, H, W] on the device (engine/test.py:140-141): the arg max, or with a region
    table (masks, values) the decoded region map (hip.region_decode_u8)"""
    if regions is not None:
        return hip.region_decode_u8(outputs[0].float().contiguous(), regions[1])
    return hip.argmax_u8(outputs[0].float().contiguous())


def region_lut(mask: int, device) -> torch.Tensor:
    """uint8 [256]: 1 where the label value belongs to the region of bit mask `mask`, for `lut[label_map.long()]`"""
    return torch.tensor([(mask >> v) & 1 if v < 32 else 0 for v in range(256)], dtype=torch.uint8, device=device)


def region_hausdorff95(maps: torch.Tensor, labels: torch.Tensor, masks) -> np.ndarray:
    """metrics.hausdorff95 per region: [B, R], both maps taken through each region's label set to {0, 1} (a cold path: a
    torch index per region), class 1 of the two-class call"""
    cols = []
    for m in masks:
        lut = region_lut(m, maps.device)
        cols.append(np.asarray(metrics.hausdorff95(lut[maps.long()], lut[labels.long()], 2))[:, 1])
    return np.stack(cols, axis=1)


def post_enabled(cfg) -> bool:
    """any post-processing flag is set"""
    return bool(getattr(cfg, "post_keep_largest", False)) or int(getattr(cfg, "post_min_size", 0)) > 1 \
        or bool(getattr(cfg, "post_fill_holes", False))


def postprocess(seg: torch.Tensor, cfg, return_stats: bool = False):
    """uint8 [D, H, W] label map -> the map after the steps the --post_* flags ask for (hip.postprocess_u8)"""
    return hip.postprocess_u8(seg, n_label_values(cfg), min_size=int(getattr(cfg, "post_min_size", 0)),
                              keep_largest=bool(getattr(cfg, "post_keep_largest", False)),
                              connectivity=int(getattr(cfg, "post_connectivity", 26)),
                              fill_holes=bool(getattr(cfg, "post_fill_holes", False)),
                              hole_connectivity=int(getattr(cfg, "post_hole_connectivity", 26)), return_stats=return_stats)


def dice_of_maps(maps: torch.Tensor, labels: torch.Tensor, n_classes: int, regions=None) -> float:
    """hard Dice of uint8 maps [B, D, H, W] against labels [B, 1, D, H, W]: per class the mean over the volumes that hold
    it, then the mean over the classes.  regions (masks, values): per region instead, from hip.region_counts_u8."""
    if regions is not None:
        from ..losses import dice_from_counts
        counts = torch.stack([hip.region_counts_u8(maps[b].contiguous(), labels[b].to(torch.uint8).contiguous(), regions[0])
                              for b in range(maps.shape[0])])
        dice = dice_from_counts(counts)[0].cpu()
        return float(torch.stack([dice[:, c].nanmean() for c in range(dice.shape[1])]).nanmean())
    dice = torch.cat([metrics.dice_from_maps(maps[b], labels[b], n_classes)[0] for b in range(maps.shape[0])]).cpu()
    return float(torch.stack([dice[:, c].nanmean() for c in range(n_classes)]).nanmean())


def _stats_line(stats, cfg) -> str:
    """the per-class counts of postprocess()' stats; with --post_keep_largest alone, the line of earlier builds"""
    min_size = int(getattr(cfg, "post_min_size", 0))
    largest, fill = bool(getattr(cfg, "post_keep_largest", False)), bool(getattr(cfg, "post_fill_holes", False))
    rows = []
    for c, (n, small_n, small_vox, removed, filled, final) in enumerate(stats.cpu().tolist()):
        if c == 0:
            continue
        parts = [f"{n} components"] if n >= 0 else []
        if min_size > 1:
            parts.append(f"{small_n} below {min_size} voxels removed ({small_vox} voxels)")
        if largest:                                   # without the fill step the class holds what was kept
            parts.append(f"{removed} removed" if fill else f"{final} kept, {removed} removed")
        if fill:
            parts.append(f"{filled} filled, {final} voxels")
        rows.append(f"class {c}: " + ", ".join(parts))
    return ", ".join(rows)


def eval_model(inferer, model, data_loader, criterion, device, cfg, log_writer=None):
    """`inferer(inputs=..., network=...)` -> logits (MONAI SlidingWindowInferer call convention, engine/test.py:47), or
    None for the built-in sliding window with the validation settings.  Returns {'eval/<meter>': global average}."""
    model.eval()
    metric_logger = misc.MetricLogger(delimiter="  ")
    post = post_enabled(cfg)
    regions = region_table(cfg)

    def hd95(maps):
        if regions is not None:
            return region_hausdorff95(maps, labels, regions[0])
        return metrics.hausdorff95(maps, labels, cfg.output_dim)

    for name in ["loss", "mHdorffDist", "mDice"] + ["class" + str(c) + "Dice" for c in range(cfg.output_dim)] \
            + (["ppDice", "ppHdorffDist"] if post else []):
        metric_logger.add_meter(name, misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    header = "Evaluation starting"
    for data_iter_step, batch in enumerate(metric_logger.log_every(data_loader, 1, header)):
        inputs = batch["image"].to(device, non_blocking=True)
        labels = batch["label"].to(device, non_blocking=True)
        aff_xyz = misc.get_affine_xyz(batch["image_meta_dict"]["original_affine"]).float().to(device)
        img_name = os.path.split(str(batch["image_meta_dict"]["filename_or_obj"][0]))[-1]
        with torch.no_grad():
            if inferer is None:
                outputs = sliding_window_inference(inputs, aff_xyz, cfg.vol_size, cfg.batch_size_val, model,
                                                   overlap=cfg.val_infer_overlap, mode="gaussian",
                                                   mirror_axes=getattr(cfg, "infer_mirror_axes", ()))
            else:
                # the reference hands the bare module to MONAI's inferer, which feeds it a bare window tensor (the models
                # want the (window, centers, affine) tuple: SURVEY.md M4); an inferer that already builds the tuple passes
                outputs = inferer(inputs=inputs, network=lambda w, *a, **k: model(
                    w if isinstance(w, (tuple, list)) else (w, None, aff_xyz)))
            loss = criterion(outputs, labels)
        mDice = _metric_update(metric_logger, criterion, outputs, labels, cfg.output_dim)
        # engine/test.py:31,48-51: Hausdorff-95 of the arg-max map against the labels, all classes, MONAI's "mean" reduction
        pred_maps = torch.stack([label_map(outputs[b:b + 1], regions) for b in range(outputs.shape[0])])
        hdorf, _ = metrics.hausdorff_mean(hd95(pred_maps))
        metric_logger.update(loss=loss.item(), mHdorffDist=hdorf, mDice=mDice.item())
        if post:
            # the same two metrics after the clean-up step; the meters above stay those of the unfiltered output
            pp_maps = torch.stack([postprocess(m, cfg) for m in pred_maps])
            pp_hdorf, _ = metrics.hausdorff_mean(hd95(pp_maps))
            metric_logger.update(ppDice=dice_of_maps(pp_maps, labels, cfg.output_dim, regions), ppHdorffDist=pp_hdorf)
        if getattr(cfg, "save_eval_output", False) and cfg.output_dir:
            os.makedirs(cfg.output_dir, exist_ok=True)
            saved = pp_maps[0] if post else pred_maps[0]
            np.save(os.path.join(cfg.output_dir, "pred_" + img_name + ".npy"), saved.cpu().numpy())
    metric_logger.synchronize_between_processes()
    print("Evaluation averaged stats:", metric_logger.log_all_average())
    return {"eval/" + k: meter.global_avg for k, meter in metric_logger.meters.items()}


def test_model(model, data_loader, device, cfg, log_writer=None):
    model.eval()
    air_cval = (0.0 - cfg.t_norm_mean) / cfg.t_norm_std if cfg.t_normalize else 0.0
    restore_mode = getattr(cfg, "restore_mode", "nearest")
    regions = region_table(cfg)
    if regions is not None and restore_mode == "linear":
        raise ValueError("--restore_mode linear is not implemented under --label_regions (the sigmoid threshold would have to "
                         "be taken per native voxel inside the restore kernel): use --restore_mode nearest, which restores "
                         "the decoded region map")
    only_largest = not (int(getattr(cfg, "post_min_size", 0)) > 1 or getattr(cfg, "post_fill_holes", False))
    for i, batch in enumerate(data_loader):
        inputs = batch["image"].to(device, non_blocking=True)
        aff_xyz = misc.get_affine_xyz(batch["image_meta_dict"]["original_affine"]).float().to(device)
        img_name = output_name(batch["image_meta_dict"]["filename_or_obj"][0])
        restore = batch.get("restore") if isinstance(batch, dict) else None
        with torch.no_grad():
            outputs = sliding_window_inference(inputs, aff_xyz, cfg.vol_size, cfg.batch_size_val, model,
                                               overlap=cfg.val_infer_overlap, mode="gaussian",
                                               cval=normalised_zero(cfg) if restore is not None else air_cval,
                                               mirror_axes=getattr(cfg, "infer_mirror_axes", ()))
        seg = label_map(outputs, regions)
        # with --restore_mode linear the clean-up runs on the native map instead (below); pred/ stays the raw arg max
        if post_enabled(cfg) and not (restore is not None and restore_mode == "linear"):
            seg, stats = postprocess(seg, cfg, return_stats=True)
            print(("keep largest component, " if only_largest else "post-processing, ") + img_name + ": "
                  + _stats_line(stats, cfg))
        seg_native = None
        if restore is not None:
            # the file's own grid: one launch undoes pad, foreground crop, spacing and orientation (hip.restore_native_u8)
            if restore_mode == "linear":
                # the sliding window blends in fp32 and returns its accumulator: no copy is made here (a view of it only when
                # the case is smaller than the window, which --t_spatial_pad rules out); another dtype would mean a hidden
                # [C][model] fp32 copy, so it is refused
                if outputs.dtype != torch.float32:
                    raise TypeError(f"--restore_mode linear reads fp32 logits, the sliding window returned {outputs.dtype}")
                seg_native = hip.restore_native_u8(outputs[0].contiguous(), restore, "linear")
                if post_enabled(cfg):
                    seg_native, stats = postprocess(seg_native, cfg, return_stats=True)
                    print(("keep largest component, " if only_largest else "post-processing, ") + img_name + " (native grid): "
                          + _stats_line(stats, cfg))
            else:
                seg_native = hip.restore_native_u8(seg, restore, "nearest")
        seg_rs = None
        if getattr(cfg, "t_voxel_spacings", None):
            target = None
            for t in batch.get("image_transforms", []):
                if t["class"][0] == "Spacingd":
                    target = [int(v[0]) if hasattr(v, "__len__") else int(v) for v in t["orig_size"]]
            if target is not None:
                seg_rs = hip.resample_nearest_u8(seg, target)
        if getattr(cfg, "save_eval_output", False) and cfg.output_dir:
            out_dir = os.path.join(cfg.output_dir, "test_output", "Fold" + str(getattr(cfg, "cv_fold", 0)))
            meta = batch["image_meta_dict"]
            aff = _affine0(meta.get("affine"))                       # translation zeroed, as engine/test.py:151-152 does
            _save_volume(os.path.join(out_dir, "pred"), img_name, seg.cpu().numpy(), aff)
            if img_name.endswith((".nii", ".nii.gz")):
                _save_volume(os.path.join(out_dir, "img"), img_name, inputs.squeeze().float().cpu().numpy(), aff)
            if seg_rs is not None:
                _save_volume(os.path.join(out_dir, "rs"), img_name, seg_rs.cpu().numpy(), _affine0(meta.get("original_affine")))
            if seg_native is not None:
                # the file's full affine, translation kept: the map overlays the input in a viewer
                full = restore["original_affine"] if "original_affine" in restore else meta["original_affine"]
                full = np.array(torch.as_tensor(full).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 4, 4)[0]
                _save_volume(os.path.join(out_dir, "native"), img_name, seg_native.cpu().numpy(), full)
        if restore is not None:
            # a file case is as large as its scan: let go of its tensors before the loader preprocesses the next one
            del batch, inputs, outputs, seg, seg_native, seg_rs
    return None


def _affine0(a):
    """first affine of the batch with its translation set to zero (/root/reference/engine/test.py:151-152); identity when
    the loader carries none"""
    if a is None:
        return np.eye(4)
    a = np.array(torch.as_tensor(a).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 4, 4)[0]
    a[0:3, 3] = 0
    return a


def _save_volume(folder, name, arr, affine):
    """NIfTI-1 (what nib.save(nib.Nifti1Image(arr, affine), path) writes, /root/reference/engine/test.py:160-170) for
    names that carry a NIfTI extension, .npy otherwise (synthetic loaders)"""
    os.makedirs(folder, exist_ok=True)
    if name.endswith((".nii", ".nii.gz")):
        from ..utils.nifti import save_nifti
        save_nifti(os.path.join(folder, name), arr, affine)
    else:
        np.save(os.path.join(folder, name + ".npy"), arr)


def majority_vote(fold_maps, n_classes: int) -> torch.Tensor:
    """fold_maps: sequence of uint8 [D, H, W] label maps (one per fold) -> voted uint8 map on the device
    (/root/reference/majority_vote.py:23-37)"""
    stack = torch.stack([torch.as_tensor(m, dtype=torch.uint8) for m in fold_maps]).contiguous()
    if not stack.is_cuda:
        stack = stack.cuda()
    return hip.majority_vote_u8(stack, n_classes)
