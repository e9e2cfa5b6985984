"""Checker of ``metrics.surface_metrics`` and of the two entry points under it: surface distances in millimetres on the
scipy.ndimage functions that ``oracle/postproc.py`` already uses for the Hausdorff distance.

* edges: ``binary_erosion(mask) ^ mask`` (default 6-neighbour structure, border value 0): MONAI's ``get_mask_edges``;
* distances: ``distance_transform_edt(~edges_other, sampling=spacing)[edges_this]``: MONAI's ``get_surface_distance``;
* ``hd_mm`` as ``compute_hausdorff_distance(percentile=q)``, ``assd_mm`` as ``compute_average_surface_distance(symmetric=
  True)``, ``nsd`` as ``compute_surface_dice`` (counts of surface voxels within the class's tolerance).

MONAI is not installed: restated from its published definitions, **parity with MONAI itself unpinned**.  The conventions
for missing classes are this project's (``surface_metrics``' docstring): a class in neither map -> NaN, NaN, NaN; a class
in exactly one map -> inf, inf, 0.  Checker only, CPU, never on a hot path."""
from __future__ import annotations

import numpy as np


def edges(mask: np.ndarray) -> np.ndarray:
    from scipy.ndimage import binary_erosion
    return binary_erosion(mask) ^ mask


def directed_distances(edges_this: np.ndarray, edges_other: np.ndarray, spacing) -> np.ndarray:
    """distance (mm) of every voxel of edges_this to the nearest voxel of edges_other, in flat (C) order of the voxels;
    all inf when edges_other is empty"""
    from scipy.ndimage import distance_transform_edt
    if not edges_other.any():
        return np.full(int(edges_this.sum()), np.inf)
    return distance_transform_edt(~edges_other, sampling=[float(s) for s in spacing])[edges_this]


def class_distances(pred: np.ndarray, label: np.ndarray, c: int, spacing):
    """-> (d_pg, d_gp, edges of pred, edges of label) for class c"""
    ep, eg = edges(pred == c), edges(label == c)
    return directed_distances(ep, eg, spacing), directed_distances(eg, ep, spacing), ep, eg


def surface_metrics_ref(pred: np.ndarray, label: np.ndarray, n_classes: int, spacing, nsd_tolerance, percentile: float = 95.0):
    """pred, label: integer maps [D, H, W] -> {"hd_mm", "assd_mm", "nsd"}: float64 [n_classes]"""
    tau = np.broadcast_to(np.asarray(nsd_tolerance, dtype=np.float64).reshape(-1), (n_classes,))
    out = {k: np.full(n_classes, np.nan, dtype=np.float64) for k in ("hd_mm", "assd_mm", "nsd")}
    for c in range(n_classes):
        has_p, has_g = bool((pred == c).any()), bool((label == c).any())
        if not has_p and not has_g:
            continue
        if not has_p or not has_g:
            out["hd_mm"][c], out["assd_mm"][c], out["nsd"][c] = np.inf, np.inf, 0.0
            continue
        d_pg, d_gp, _, _ = class_distances(pred, label, c, spacing)
        n = d_pg.size + d_gp.size
        out["hd_mm"][c] = max(np.percentile(d_pg, percentile), np.percentile(d_gp, percentile))
        out["assd_mm"][c] = (d_pg.sum() + d_gp.sum()) / n
        out["nsd"][c] = ((d_pg <= tau[c]).sum() + (d_gp <= tau[c]).sum()) / n
    return out


# an anisotropic grid with two flipped axes and a translation: spacing (0.8, 0.8, 5.0) mm along the array axes
SCORE_AFFINE = np.array([[-0.8, 0.0, 0.0, 91.5], [0.0, -0.8, 0.0, -17.25], [0.0, 0.0, 5.0, -310.0], [0.0, 0.0, 0.0, 1.0]])


def write_score_task(root, labels, preds, affine=SCORE_AFFINE, task="Task77_Score"):
    """a temporary Decathlon task for run_score.py: labels / preds = {case id: uint8 [X, Y, Z]}; label files go to
    <root>/<task>/labelsTr/<id>.nii.gz and into the "training" section (image names imagesTr/img<id>.nii.gz, not
    written: the scorer reads no image), predictions to <root>/pred/<id>.nii.gz -> (data_path, task, pred_folder)"""
    import json
    import os

    from medicalsemseg_amd.utils.nifti import save_nifti
    tdir, pdir = os.path.join(str(root), task), os.path.join(str(root), "pred")
    os.makedirs(os.path.join(tdir, "labelsTr"), exist_ok=True)
    os.makedirs(pdir, exist_ok=True)
    for cid, lab in labels.items():
        save_nifti(os.path.join(tdir, "labelsTr", f"{cid}.nii.gz"), lab, affine)
    for cid, pr in preds.items():
        save_nifti(os.path.join(pdir, f"{cid}.nii.gz"), pr, affine)
    js = {"training": [{"image": f"./imagesTr/img{cid}.nii.gz", "label": f"./labelsTr/{cid}.nii.gz"} for cid in labels],
          "test": ["./imagesTs/imgt0.nii.gz"]}
    with open(os.path.join(tdir, "dataset.json"), "w") as f:
        json.dump(js, f)
    return str(root), task, pdir
