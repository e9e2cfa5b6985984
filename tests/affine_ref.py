"""numpy restatement of msseg_aug_crop_affine (include/msseg.h): the device crop gather sampling a cached volume under a 3x3
matrix per patch.  Coordinates in float64 with one rounding per operation in the stated order, interpolation in float32
lerps a + f * (b - a) along x, then y, then z; a tap outside the volume reads the pad value (scipy's mode="grid-constant"),
the label is the nearest voxel floor(c + 0.5), 0 outside.  Checked against scipy.ndimage.affine_transform in
tests/test_affine_host.py."""
from __future__ import annotations

import numpy as np


def patch_index(roi, flips, rotk):
    """output voxel grid -> patch index (sz, sy, sx): the quarter turn in the (z, y) plane (np.rot90 sense) and the flip
    bits (bit 0 / 1 / 2 = axis d / h / w) undone"""
    z, y, x = np.indices((roi,) * 3)
    sz, sy = z, y
    if rotk == 1:
        sz, sy = y, roi - 1 - z
    elif rotk == 2:
        sz, sy = roi - 1 - z, roi - 1 - y
    elif rotk == 3:
        sz, sy = roi - 1 - y, z
    if flips & 1:
        sz = roi - 1 - sz
    if flips & 2:
        sy = roi - 1 - sy
    sx = roi - 1 - x if flips & 4 else x
    return sz, sy, sx


def clamp_start(start, roi, shape):
    return tuple(min(max(int(s), 0), n - roi) for s, n in zip(start, shape))


def source_coords(start, roi, flips, rotk, mat):
    """float64 [3, R, R, R]: c[a] = (start[a] + h) + ((M[a][0] d[0] + M[a][1] d[1]) + M[a][2] d[2]), h = (R - 1) / 2, d = p - h"""
    m = np.asarray(mat, dtype=np.float64).reshape(3, 3)
    h = (roi - 1) / 2.0
    d = [p.astype(np.float64) - h for p in patch_index(roi, flips, rotk)]
    return np.stack([(float(start[a]) + h) + ((m[a, 0] * d[0] + m[a, 1] * d[1]) + m[a, 2] * d[2]) for a in range(3)])


def sample_image(img, c, pad):
    """img float32 [C, D, H, W], c float64 [3, ...] -> float32 [C, ...]: 8 taps at floor(c), lerps along x, y, z in float32"""
    img = np.asarray(img, dtype=np.float32)
    shape = img.shape[1:]
    i = np.floor(c)
    f = (c - i).astype(np.float32)
    i = i.astype(np.int64)
    pad = np.float32(pad)

    def tap(oz, oy, ox):
        idx = [i[0] + oz, i[1] + oy, i[2] + ox]
        ok = np.ones(idx[0].shape, dtype=bool)
        for a in range(3):
            ok &= (idx[a] >= 0) & (idx[a] < shape[a])
        idx = [np.clip(idx[a], 0, shape[a] - 1) for a in range(3)]
        return np.where(ok[None], img[:, idx[0], idx[1], idx[2]], pad).astype(np.float32)

    fz, fy, fx = f[0][None], f[1][None], f[2][None]
    t000, t001, t010, t011 = tap(0, 0, 0), tap(0, 0, 1), tap(0, 1, 0), tap(0, 1, 1)
    t100, t101, t110, t111 = tap(1, 0, 0), tap(1, 0, 1), tap(1, 1, 0), tap(1, 1, 1)
    v00, v01 = t000 + fx * (t001 - t000), t010 + fx * (t011 - t010)
    v10, v11 = t100 + fx * (t101 - t100), t110 + fx * (t111 - t110)
    v0, v1 = v00 + fy * (v01 - v00), v10 + fy * (v11 - v10)
    out = v0 + fz * (v1 - v0)
    assert out.dtype == np.float32
    return out


def sample_label(lab, c):
    """lab [D, H, W] or None, c float64 [3, ...] -> float32 [...]: the voxel floor(c + 0.5), 0 outside or without a label"""
    if lab is None:
        return np.zeros(c.shape[1:], dtype=np.float32)
    n = np.floor(c + 0.5).astype(np.int64)
    ok = np.ones(n[0].shape, dtype=bool)
    for a in range(3):
        ok &= (n[a] >= 0) & (n[a] < lab.shape[a])
    n = [np.clip(n[a], 0, lab.shape[a] - 1) for a in range(3)]
    return np.where(ok, lab[n[0], n[1], n[2]], 0).astype(np.float32)


def affine_crop(img, lab, start, roi, flips, rotk, shift, scale, mat, pad):
    """one row of msseg_aug_crop_affine: img float32 [C, D, H, W], lab [D, H, W] or None, start = the pick table's crop start,
    flips = the bit mask, shift / scale as the row's fp32 fields -> (float32 [C, R, R, R], float32 [R, R, R])"""
    start = clamp_start(start, roi, img.shape[1:])
    c = source_coords(start, roi, flips, rotk, mat)
    v = sample_image(img, c, pad)
    v = (v + np.float32(shift)).astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(v.astype(np.float32)), sample_label(lab, c)


def half_integer_share(c, eps=1e-6):
    """share of the voxels with a coordinate within eps of a half-integer: there nearest-voxel rules may disagree"""
    frac = c - np.floor(c)
    return float(np.mean(np.any(np.abs(frac - 0.5) < eps, axis=0)))


def random_matrix(rng, max_deg=30.0, zoom=(0.7, 1.4)):
    from medicalsemseg_amd.data_device import affine_matrix
    ang = np.deg2rad(rng.uniform(-max_deg, max_deg, 3))
    return affine_matrix(ang, float(rng.uniform(*zoom)))
