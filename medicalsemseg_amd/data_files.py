"""Host side of the dataset path: Decathlon datalist, cross-validation split, per-rank partition, orientation and shape
arithmetic.  Restates what the reference does with MONAI in ``data/dataset_builder.py:431-464`` (``load_decathlon_datalist``,
the seeded shuffle + ``np.array_split`` folds, ``partition_dataset(shuffle=False, even_divisible=True)``) and the geometry of
``Orientationd(axcodes="RAS")`` / ``Spacingd`` (``:19-36``).  MONAI and nibabel are absent: MONAI parity unpinned; the rules
below are the published semantics as recalled and are pinned by ``tests/test_data_host.py`` only against themselves.
File I/O and a few 4x4 matrices: out of the GPU hot path."""
from __future__ import annotations

import json
import os
import random

import numpy as np


def _resolve(base, p):
    return p if os.path.isabs(p) else os.path.normpath(os.path.join(base, p))


def datalist_path(data_path, task, json_list):
    return os.path.join(data_path, task, json_list)


def has_key(json_path, key):
    with open(json_path) as f:
        return key in json.load(f)


def load_datalist(json_path, key="training"):
    """``{key: [{"image": ..., "label": ...}, ...]}`` -> list of dicts; relative paths are joined to the JSON's directory"""
    with open(json_path) as f:
        js = json.load(f)
    if key not in js:
        raise ValueError(f'data list {json_path} has no "{key}" section')
    base = os.path.dirname(os.path.abspath(json_path))
    out = []
    for item in js[key]:
        if isinstance(item, str):               # image-only sections (Decathlon "test")
            item = {"image": item}
        out.append({k: (_resolve(base, v) if k in ("image", "label") and isinstance(v, str) else v) for k, v in item.items()})
    return out


def cv_split(files, seed, cv_max_folds, cv_fold):
    """dataset_builder.py:441-448: seeded in-place shuffle, np.array_split into folds, fold cv_fold validates"""
    files = list(files)
    random.Random(seed).shuffle(files)
    splits = np.array_split(files, cv_max_folds)
    folds = list(range(cv_max_folds))
    folds.pop(cv_fold)
    train = [f for i in folds for f in splits[i]]
    return train, list(splits[cv_fold])


def partition(files, num_partitions, rank, even_divisible=True):
    """MONAI partition_dataset(shuffle=False): indices padded with their own head to a multiple of num_partitions when
    even_divisible, rank r takes indices[r::num_partitions]"""
    idx = list(range(len(files)))
    if even_divisible and idx and len(idx) % num_partitions:
        need = num_partitions - len(idx) % num_partitions
        while need > 0:
            take = idx[:need] if need <= len(idx) else list(idx)
            idx += take
            need -= len(take)
    return [files[i] for i in idx[rank::num_partitions]]


def ras_orientation(affine):
    """-> (perm, flips): output axis o of the RAS volume is input axis perm[o], reversed when flips[o]; the dominant world
    axis of every voxel axis, largest components first so that no world axis is taken twice"""
    M = np.asarray(affine, dtype=np.float64)[:3, :3]
    norm = np.sqrt((M * M).sum(0))
    norm[norm == 0] = 1.0
    A = np.abs(M / norm)
    perm, flips = [None] * 3, [False] * 3
    for _ in range(3):
        o, i = np.unravel_index(np.argmax(A), A.shape)
        perm[o], flips[o] = int(i), bool(M[o, i] < 0)
        A[o, :] = -1.0
        A[:, i] = -1.0
    return tuple(perm), tuple(flips)


def reorient_affine(affine, shape, perm, flips):
    """affine of the volume after transpose(perm) and the flips (shape: spatial shape before)"""
    aff = np.asarray(affine, dtype=np.float64)
    out = np.eye(4)
    out[:3, 3] = aff[:3, 3]
    for o in range(3):
        col = aff[:3, perm[o]]
        if flips[o]:
            out[:3, 3] += col * (shape[perm[o]] - 1)
            col = -col
        out[:3, o] = col
    return out


def spacing_of(affine):
    M = np.asarray(affine, dtype=np.float64)[:3, :3]
    return np.sqrt((M * M).sum(0))


def resample_shape(n, old, new):
    """output length of one axis under Spacingd: round((n - 1) * old / new + 1) (MONAI compute_shape_offset as recalled:
    unpinned)"""
    return max(int(np.round((n - 1) * float(old) / float(new) + 1.0)), 1)


def rescale_affine(affine, ratio):
    """columns scaled by ratio = new / old spacing per axis (voxel 0 stays voxel 0)"""
    out = np.array(affine, dtype=np.float64)
    out[:3, :3] = out[:3, :3] * np.asarray(ratio, dtype=np.float64)[None, :]
    return out


def shift_affine(affine, start):
    """affine of a crop that starts at voxel `start` (negative: padding in front)"""
    out = np.array(affine, dtype=np.float64)
    out[:3, 3] = out[:3, 3] + out[:3, :3] @ np.asarray(start, dtype=np.float64)
    return out


def load_case(item):
    """-> (image [C, X, Y, Z] native dtype, label [X, Y, Z] uint8 or None, affine); a 4-D image has its channels last on file"""
    from .utils.nifti import load_nifti
    img, aff = load_nifti(item["image"])
    if img.ndim == 3:
        img = img[None]
    elif img.ndim == 4:
        img = np.moveaxis(img, -1, 0)
    else:
        raise ValueError(f"{item['image']}: 3-D or 4-D (channels last) image expected, got shape {img.shape}")
    lab = None
    if item.get("label"):
        lab, _ = load_nifti(item["label"])
        if lab.shape != img.shape[1:]:
            raise ValueError(f"{item['label']}: label shape {lab.shape} differs from the image's {img.shape[1:]}")
        lab = np.ascontiguousarray(lab).astype(np.uint8)
    return np.ascontiguousarray(img), lab, aff
