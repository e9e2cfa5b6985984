"""torch restatement, on the CPU, of sliding-window inference with mirror test-time augmentation
(medicalsemseg_amd.engine.utils.sliding_window_inference(..., mirror_axes=...)): the loop of oracle/sliding_window.py with
every window start repeated once per flip mask, mask fastest.  A row's window is `torch.flip` of the plain window, the
predictor sees it with the window's own `centers` row, its logits are flipped back and blended like any other row:
`out[sl] += imp * seg; cnt[sl] += imp`, row by row, then `out / cnt`.  The weight map is never flipped.  With one mask it
is the oracle's loop, bit for bit (tests/test_sw_mirror_host.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from medicalsemseg_amd.engine.utils import (fall_back_tuple, get_scan_interval, importance_map, mirror_masks,
                                            window_starts)


def flip_dims(mask, first_spatial_dim):
    """the tensor dims a mask flips: bit a = volume axis a (0 = D, 1 = H, 2 = W)"""
    return [first_spatial_dim + a for a in range(3) if mask >> a & 1]


def sliding_window_mirror_ref(inputs, affine, roi_size, sw_batch_size, predictor, overlap=0.25, mode="constant",
                              sigma_scale=0.125, cval=0.0, mirror_axes=()):
    """inputs: fp32 NCDHW on the CPU -> fp32 [N, classes, D, H, W]"""
    image_size_ = list(inputs.shape[2:])
    B = inputs.shape[0]
    roi = fall_back_tuple(roi_size, image_size_)
    image_size = tuple(max(image_size_[d], roi[d]) for d in range(3))
    pad = []
    for d in (2, 1, 0):
        diff = max(roi[d] - image_size_[d], 0)
        pad += [diff // 2, diff - diff // 2]
    vol = F.pad(inputs.float(), pad=pad, mode="constant", value=cval)
    starts = window_starts(image_size, roi, get_scan_interval(image_size, roi, 3, overlap))
    imp = importance_map(tuple(min(r, i) for r, i in zip(roi, image_size)), mode, sigma_scale)
    masks = mirror_masks(mirror_axes)
    rows = [(b, st, m) for b in range(B) for st in starts for m in masks]
    out = cnt = None
    for g in range(0, len(rows), sw_batch_size):
        batch = rows[g:g + sw_batch_size]
        sls = [(slice(b, b + 1), slice(None)) + tuple(slice(st[d], st[d] + roi[d]) for d in range(3)) for b, st, _ in batch]
        centers = torch.tensor([[(st[d] + roi[d] - roi[d] // 2) / image_size[d] for d in range(3)] for _, st, _ in batch],
                               dtype=torch.float32)
        if sw_batch_size == 1:
            centers = centers.unsqueeze(0)
        win = torch.cat([torch.flip(vol[sl], flip_dims(m, 2)) for sl, (_, _, m) in zip(sls, batch)])
        seg = predictor((win, centers, affine))
        if out is None:
            out = torch.zeros(B, seg.shape[1], *image_size, dtype=torch.float32)
            cnt = torch.zeros(B, 1, *image_size, dtype=torch.float32)
        for k, (sl, (_, _, m)) in enumerate(zip(sls, batch)):
            out[sl] += imp * torch.flip(seg[k], flip_dims(m, 1))
            cnt[sl] += imp
    out = out / cnt
    lo = [max(roi[d] - image_size_[d], 0) // 2 for d in range(3)]
    return out[:, :, lo[0]:lo[0] + image_size_[0], lo[1]:lo[1] + image_size_[1], lo[2]:lo[2] + image_size_[2]]
