"""numpy / scipy restatement of the class-ratio crop centres (csrc/class_crop.hip, data_device.DeviceDatasetLoader with
crop="class_ratios"): the candidate sets, their per-slice counts, the k-th candidate in flat order and the row a pick
writes.  Voxel v is a candidate of class c iff image_ok(img0(v)) and a voxel of label c lies within L1 distance n of v:
scipy's binary_dilation(lab == c, iterations=n) with the default (6-neighbour) structure."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

from medicalsemseg_amd.data_device import correct_crop_center


def image_ok(img0, thr=0.0, rule="gt"):
    return img0 != np.float32(thr) if rule == "ne" else img0 > np.float32(thr)


def dilate(mask, n):
    """the voxels within L1 distance n of a voxel of `mask`"""
    mask = np.asarray(mask, dtype=bool)
    return ndimage.binary_dilation(mask, iterations=int(n)) if n > 0 else mask.copy()


def dilate_brute(mask, n):
    """the same from the definition: every voxel against every voxel of the mask"""
    mask = np.asarray(mask, dtype=bool)
    pts = np.argwhere(mask)
    out = np.zeros(mask.shape, dtype=bool)
    for v in np.ndindex(*mask.shape):
        out[v] = pts.size > 0 and int(np.abs(pts - np.array(v)).sum(1).min()) <= n
    return out


def candidates(img0, lab, c, n=0, thr=0.0, rule="gt"):
    """bool [D, H, W]: the crop-centre candidates of class c"""
    return dilate(lab == c, n) & image_ok(img0, thr, rule)


def candidate_mask(img0, lab, classes, n, thr=0.0, rule="gt"):
    """uint16 [D, H, W]: bit c = candidates(..., c, n) for the classes asked for, 0 for the others"""
    out = np.zeros(lab.shape, dtype=np.uint16)
    for c in classes:
        out |= candidates(img0, lab, c, n, thr, rule).astype(np.uint16) << np.uint16(c)
    return out


def slab_counts(img0, lab, n_classes, n=0, thr=0.0, rule="gt", classes=None):
    """int32 [D, n_classes]: candidates per z-slice and class (classes: those built when n > 0; the others count 0)"""
    out = np.zeros((lab.shape[0], n_classes), dtype=np.int32)
    for c in (range(n_classes) if classes is None else classes):
        out[:, c] = candidates(img0, lab, c, n, thr, rule).reshape(lab.shape[0], -1).sum(1)
    return out


def kth_in_slice(cand, z, k):
    """in-slice flat index of the k-th candidate (flat order) of slice z, -1 when the slice has no more than k"""
    idx = np.flatnonzero(cand[z])
    return int(idx[k]) if 0 <= k < idx.size else -1


def pick_row(shape, z, hit, roi):
    """the 8 ints a pick writes: clamped centre, crop start, z, in-slice flat index (-1: the centre of voxel (z, 0, 0))"""
    D, H, W = shape
    y, x = (hit // W, hit % W) if hit >= 0 else (0, 0)
    c = correct_crop_center((z, y, x), (roi,) * 3, shape)
    return [*c, *(v - roi // 2 for v in c), z, hit]
