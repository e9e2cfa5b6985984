"""Test helper: numpy / scipy restatements of the preprocessing transforms the reference chains with MONAI in
``data/dataset_builder.py:19-217, 220-306, 431-488`` and ``data/transforms.py:17-75``, plus writers for small NIfTI
fixtures.  MONAI and nibabel are absent: MONAI parity unpinned; these restate the published semantics as recalled, one
numpy operation at a time, and are what the device kernels are pinned against."""
from __future__ import annotations

import gzip
import struct

import numpy as np


# ---- intensity ------------------------------------------------------------------------------------------------------
def scale_intensity_range(img, a_min, a_max):
    """ScaleIntensityRange(a_min, a_max, 0, 1, clip=True) on float32, one rounding per operation"""
    x = np.asarray(img).astype(np.float32)
    x = (x - np.float32(a_min)) / np.float32(a_max - a_min)
    x = x * np.float32(1.0) + np.float32(0.0)
    return np.clip(x, np.float32(0.0), np.float32(1.0)).astype(np.float32)


def scale_cubed_intensity_range64(img, a_min, a_max):
    """ScaleCubedIntensityRange (transforms.py:45-75) in float64: cbrt of the value and of both bounds, same map and clip"""
    x = np.cbrt(np.asarray(img).astype(np.float64))
    lo, hi = np.cbrt(float(a_min)), np.cbrt(float(a_max))
    return np.clip((x - lo) / (hi - lo), 0.0, 1.0)


def normalize_intensity(img, subtrahend, divisor):
    return ((np.asarray(img, dtype=np.float32) - np.float32(subtrahend)) / np.float32(divisor)).astype(np.float32)


def foreground_box(img):
    """CropForeground(select_fn = x > 0) over [C, D, H, W]: (z0, y0, x0, z1, y1, x1) half-open; None when empty"""
    nz = np.nonzero((np.asarray(img) > 0).any(0))
    if nz[0].size == 0:
        return None
    return tuple(int(a.min()) for a in nz) + tuple(int(a.max()) + 1 for a in nz)


# ---- spacing --------------------------------------------------------------------------------------------------------
def resample_shape(n, old, new):
    return max(int(np.round((n - 1) * float(old) / float(new) + 1.0)), 1)


def resample_coords(out_shape, ratio):
    """source coordinates (float64) of every output voxel: index * new / old per axis"""
    return np.meshgrid(*[np.arange(n, dtype=np.float64) * float(r) for n, r in zip(out_shape, ratio)], indexing="ij")


def resample_image64(img, out_shape, ratio):
    """trilinear with border clamping, float64: scipy.ndimage.map_coordinates(order=1, mode="nearest")"""
    from scipy.ndimage import map_coordinates
    co = resample_coords(out_shape, ratio)
    return np.stack([map_coordinates(np.asarray(c, dtype=np.float64), co, order=1, mode="nearest") for c in img])


def resample_label(lab, out_shape, ratio):
    """nearest: floor(coordinate + 0.5), clamped to the volume (scipy's order-0 rule)"""
    idx = [np.clip(np.floor(np.arange(n, dtype=np.float64) * float(r) + 0.5).astype(np.int64), 0, s - 1)
           for n, r, s in zip(out_shape, ratio, lab.shape)]
    return lab[np.ix_(*idx)]


# ---- crop + pad -----------------------------------------------------------------------------------------------------
def crop_pad(vol, box, min_size, pad_value):
    """vol [C, D, H, W]; box half-open; SpatialPad split: (target - n) // 2 before, the rest after"""
    z0, y0, x0, z1, y1, x1 = box
    v = vol[:, z0:z1, y0:y1, x0:x1]
    widths = [(0, 0)]
    for n, t in zip(v.shape[1:], min_size if min_size is not None else v.shape[1:]):
        tgt = max(n, t)
        widths.append(((tgt - n) // 2, tgt - n - (tgt - n) // 2))
    return np.pad(v, widths, mode="constant", constant_values=pad_value)


def slab_counts(img0, lab, thr):
    fg = lab > 0
    bg = (lab == 0) & (img0 > thr)
    return np.stack([fg.reshape(lab.shape[0], -1).sum(1), bg.reshape(lab.shape[0], -1).sum(1)], 1).astype(np.int32)


# ---- NIfTI fixtures -------------------------------------------------------------------------------------------------
def write_nifti_raw(path, array, *, pixdim=(1.0, 1.0, 1.0), qfac=1.0, slope=float("nan"), inter=float("nan"), qform_code=0,
                    quatern=(0.0, 0.0, 0.0), qoffset=(0.0, 0.0, 0.0), sform_code=0, srows=None):
    """a NIfTI-1 single file whose header fields are set one by one (the product's save_nifti always writes an sform)"""
    codes = {np.dtype("uint8"): (2, 8), np.dtype("int16"): (4, 16), np.dtype("float32"): (16, 32)}
    a = np.asarray(array)
    code, bits = codes[a.dtype]
    dim = [a.ndim] + list(a.shape) + [1] * (7 - a.ndim)
    pd = [float(qfac)] + [float(v) for v in pixdim] + [1.0] * (7 - len(pixdim))
    srows = np.zeros((3, 4)) if srows is None else np.asarray(srows, dtype=np.float64)
    hdr = struct.pack("<i10s18sihcB", 348, b"", b"", 0, 0, b"r", 0)
    hdr += struct.pack("<8h", *dim)
    hdr += struct.pack("<3f", 0.0, 0.0, 0.0)
    hdr += struct.pack("<4h", 0, code, bits, 0)
    hdr += struct.pack("<8f", *pd)
    hdr += struct.pack("<f", 352.0)
    hdr += struct.pack("<2f", float(slope), float(inter))
    hdr += struct.pack("<hBB", 0, 0, 0)
    hdr += struct.pack("<4f", 0.0, 0.0, 0.0, 0.0)
    hdr += struct.pack("<2i", 0, 0)
    hdr += struct.pack("<80s24s", b"", b"")
    hdr += struct.pack("<2h", int(qform_code), int(sform_code))
    hdr += struct.pack("<6f", *[float(v) for v in quatern], *[float(v) for v in qoffset])
    hdr += struct.pack("<12f", *[float(v) for v in srows.reshape(-1)])
    hdr += struct.pack("<16s4s", b"", b"n+1\0")
    assert len(hdr) == 348
    payload = hdr + b"\0\0\0\0" + a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes(order="F")
    with (gzip.open if str(path).endswith(".gz") else open)(path, "wb") as f:
        f.write(payload)


def ellipsoid_labels(shape, n_cls):
    ax = [np.linspace(-1, 1, s) for s in shape]
    r = np.sqrt(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2)
    y = np.zeros(shape, dtype=np.uint8)
    for c in range(1, n_cls):
        y[r < 0.8 * (n_cls - c) / max(n_cls - 1, 1)] = c
    return y


def write_ct_dataset(root, n=6, n_cls=2, seed=5, with_validation=False):
    """a small Decathlon-style task directory: int16 "CT" volumes of different non-cubic sizes, anisotropic spacing, one
    LPS affine, nested-ellipsoid labels, dataset.json without a "validation" section -> list of (image, label) names"""
    import json
    import os
    from medicalsemseg_amd.utils.nifti import save_nifti
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "imagesTr"), exist_ok=True)
    os.makedirs(os.path.join(root, "labelsTr"), exist_ok=True)
    shapes = [(48, 64, 56), (40, 72, 60), (44, 60, 80), (36, 56, 64), (48, 80, 52), (42, 66, 70)]
    items = []
    for i in range(n):
        shp = shapes[i % len(shapes)]
        lab = ellipsoid_labels(shp, n_cls)
        body = ellipsoid_labels(shp, 2) if n_cls > 2 else None
        img = rng.normal(-600.0, 60.0, shp)
        img[2:-2, 3:-3, 3:-3] += 500.0                             # "body" above the CT floor, a margin below it
        img = img + 300.0 * lab
        img[:2] = img[-2:] = -1024.0
        img[:, :3] = img[:, -3:] = -1024.0
        img[:, :, :3] = img[:, :, -3:] = -1024.0
        img = np.clip(np.round(img), -1024, 3000).astype(np.int16)
        aff = np.diag([1.5, 0.8, 0.8, 1.0])
        aff[:3, 3] = (-30.0, -20.0, 10.0)
        if i == 1:                                                  # LPS: first two axes point the other way
            aff = np.diag([-1.5, -0.8, 0.8, 1.0])
            aff[:3, 3] = (30.0, 20.0, 10.0)
        name = f"ct_{i:02d}.nii.gz"
        save_nifti(os.path.join(root, "imagesTr", name), img, aff)
        save_nifti(os.path.join(root, "labelsTr", name), lab, aff)
        items.append({"image": f"./imagesTr/{name}", "label": f"./labelsTr/{name}"})
    js = {"name": "synthetic CT", "training": items}
    if with_validation:
        js["training"], js["validation"] = items[:-2], items[-2:]
    with open(os.path.join(root, "dataset.json"), "w") as f:
        json.dump(js, f)
    return items
