"""Evaluation metrics that the reference takes from MONAI, on the device.

``hausdorff95``: ``HausdorffDistanceMetric(include_background=True, percentile=95, reduction="mean", get_not_nans=True)``
as ``/root/reference/engine/test.py:31,48-51,64`` builds, feeds (arg-max one-hot prediction, one-hot label) and reduces it.
MONAI's route is CPU scipy per (sample, class): bounding-box crop, ``binary_erosion`` XOR for the surfaces,
``distance_transform_edt`` of the whole box, a fancy-index read, ``np.percentile``.  Here the label maps never leave the
GPU: one pass marks the surfaces of all classes of both maps (``msseg_hd_edges``), then per class and direction three integer
line passes give the exact squared distance of every surface voxel to the other surface and a histogram of them
(``msseg_hd_directed_hist``); the host reads the two order statistics the percentile interpolates between from the
histogram (a few KB) and finishes in double -- the same values scipy / numpy produce, bit for bit (tests/test_gpu_engine.py
compares with ``oracle/postproc.py``, which calls scipy).  No CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip


def _percentile_ranks(n: int, q: float):
    """np.percentile of n values at q, method 'linear': -> (prev, nxt, t), the zero-based ranks of the two order statistics it
    interpolates between and the weight of the second (numpy's get_virtual_index and its clipping)"""
    quant = np.true_divide(q, 100.0)
    vi = (n - 1) * quant
    prev = int(np.floor(vi))
    nxt = min(prev + 1, n - 1)
    prev = max(min(prev, n - 1), 0)
    return prev, nxt, np.float64(vi - np.floor(vi))


def _lerp(a, b, t) -> float:
    """numpy's _lerp of the order statistics a <= b"""
    d = b - a
    r = a + d * t
    if t >= 0.5:
        r = b - d * (1 - t)
    return float(r)


def _percentile_from_hist(counts: np.ndarray, q: float) -> float:
    """np.percentile(sqrt(d2) for every counted d2, q) (method 'linear', numpy's own arithmetic) from counts[d2]"""
    n = int(counts.sum())
    cum = np.cumsum(counts)
    prev, nxt, t = _percentile_ranks(n, q)
    a = np.sqrt(np.float64(int(np.searchsorted(cum, prev + 1, side="left"))))    # order statistic `prev` (0-based)
    b = np.sqrt(np.float64(int(np.searchsorted(cum, nxt + 1, side="left"))))
    return _lerp(a, b, t)


def hausdorff95(pred: torch.Tensor, label: torch.Tensor, n_classes: int, percentile: float = 95.0) -> np.ndarray:
    """pred, label: integer label maps [B, D, H, W] (or [B, 1, D, H, W]) on the GPU -> hd [B, n_classes] float64 (host):
    NaN where neither map has the class and, with numpy >= 1.22's percentile, also where only one has it (MONAI's
    get_surface_distance yields all-inf distances there; see below)."""
    if not pred.is_cuda or not label.is_cuda:
        raise RuntimeError("hausdorff95 runs on the GPU only (no CPU fallback; the scipy restatement is oracle/postproc.py)")
    if pred.dim() == 5:
        pred = pred[:, 0]
    if label.dim() == 5:
        label = label[:, 0]
    pred = pred.to(torch.uint8).contiguous()
    label = label.to(torch.uint8).contiguous()
    B, D, H, W = pred.shape
    hd = np.full((B, n_classes), np.nan, dtype=np.float64)
    hist = None
    for b in range(B):
        ep, eg, stats = hip.hd_edges(pred[b], label[b], n_classes)
        st = stats.cpu().numpy()
        for c in range(n_classes):
            n_p, n_g = int(st[c, 6]), int(st[c, 7])
            if n_p == 0 and n_g == 0:
                continue                                  # class absent from both maps: NaN
            if n_p == 0 or n_g == 0:
                # one surface empty: MONAI's get_surface_distance hands np.percentile an all-inf array in both directions.
                # numpy (>= 1.22, incl. the 2.2 here) interpolates as a + (b - a) * t: inf - inf -> NaN, so the class drops
                # out of the mean like an absent one (older numpy gave inf); the same arithmetic, not a constant:
                with np.errstate(invalid="ignore"):
                    hd[b, c] = float(np.float64(np.inf) + (np.float64(np.inf) - np.float64(np.inf)) * 0.5)
                continue
            box = (int(st[c, 0]), int(st[c, 1]), int(st[c, 2]), int(st[c, 3]) + 1, int(st[c, 4]) + 1, int(st[c, 5]) + 1)
            bz, by, bx = box[3] - box[0], box[4] - box[1], box[5] - box[2]
            nbins = (bz - 1) ** 2 + (by - 1) ** 2 + (bx - 1) ** 2 + 2
            if hist is None or hist.numel() < nbins:
                hist = torch.empty(max(nbins, 1 << 16), dtype=torch.int32, device=pred.device)
            d = []
            for src, tgt in ((eg, ep), (ep, eg)):         # pred -> gt, then gt -> pred (compute_hausdorff_distance)
                hip.hd_directed_hist(src, tgt, c, box, hist[:nbins])
                counts = hist[:nbins].cpu().numpy().astype(np.int64)
                assert counts[-1] == 0, "a surface voxel found no voxel of a non-empty surface"
                d.append(_percentile_from_hist(counts[:-1], percentile))
            hd[b, c] = max(d)
    return hd


def surface_metrics(pred: torch.Tensor, label: torch.Tensor, n_classes: int, spacing, nsd_tolerance, percentile: float = 95.0):
    """Surface metrics in millimetres of ONE pair of uint8 label maps [D, H, W] on the GPU (no CPU fallback; the scipy
    restatement is tests/surface_ref.py).  spacing: three floats in tensor-axis order; nsd_tolerance: one float, or one per
    class.  -> {"hd_mm", "assd_mm", "nsd"}: float64 [n_classes] (host).  Per class, with d_pg the distances of the
    prediction's surface voxels to the label's surface and d_gp the reverse (MONAI's definitions):

    * hd_mm   = max(np.percentile(d_pg, percentile), np.percentile(d_gp, percentile)), method 'linear'
    * assd_mm = (sum d_pg + sum d_gp) / (|d_pg| + |d_gp|)         (compute_average_surface_distance(symmetric=True))
    * nsd     = (#{d_pg <= tau} + #{d_gp <= tau}) / (|d_pg| + |d_gp|)   (compute_surface_dice: voxels, not surface area)

    A class in neither map gives NaN, NaN, NaN.  A class in exactly one map gives inf, inf, 0: on purpose NOT what
    ``hausdorff95`` does, which lets such a class fall out of the mean as NaN -- a scorer must not flatter a prediction that
    missed an organ.  The distance maps stay on the device (``msseg_sd_directed_mm``); per class and direction one 128-byte
    record comes back (``msseg_sd_summary``): counts, the sum, and the two order statistics of d^2 the percentile
    interpolates between, whose square roots and lerp are taken here as ``_percentile_from_hist`` does."""
    if not pred.is_cuda or not label.is_cuda:
        raise RuntimeError("surface_metrics runs on the GPU only (no CPU fallback; the scipy restatement is "
                           "tests/surface_ref.py)")
    if pred.dim() != 3 or pred.shape != label.shape or pred.dtype != torch.uint8 or label.dtype != torch.uint8:
        raise ValueError("surface_metrics: pred and label must be uint8 maps [D, H, W] of one shape")
    spacing = [float(v) for v in spacing]
    if len(spacing) != 3:
        raise ValueError("surface_metrics: spacing must hold three values (tensor-axis order)")
    tau = np.asarray(nsd_tolerance, dtype=np.float64).reshape(-1)
    if tau.size not in (1, n_classes):
        raise ValueError(f"surface_metrics: nsd_tolerance must hold 1 or {n_classes} values")
    tau = np.broadcast_to(tau, (n_classes,))
    out = {k: np.full(n_classes, np.nan, dtype=np.float64) for k in ("hd_mm", "assd_mm", "nsd")}
    ep, eg, stats = hip.hd_edges(pred.contiguous(), label.contiguous(), n_classes)
    st = stats.cpu().numpy()
    for c in range(n_classes):
        n_p, n_g = int(st[c, 6]), int(st[c, 7])
        if n_p == 0 and n_g == 0:
            continue
        if n_p == 0 or n_g == 0:
            out["hd_mm"][c], out["assd_mm"][c], out["nsd"][c] = np.inf, np.inf, 0.0
            continue
        box = (int(st[c, 0]), int(st[c, 1]), int(st[c, 2]), int(st[c, 3]) + 1, int(st[c, 4]) + 1, int(st[c, 5]) + 1)
        hd, total, within = [], np.float64(0.0), 0
        for src, tgt, n in ((eg, ep, n_p), (ep, eg, n_g)):    # pred -> gt, then gt -> pred
            prev, nxt, t = _percentile_ranks(n, percentile)
            rec = hip.sd_summary(hip.sd_directed_mm(src, tgt, c, box, spacing), [tau[c]], [prev, nxt])
            assert rec.n == n and rec.n_inf == 0, "a surface voxel found no voxel of a non-empty surface"
            a, b = np.sqrt(rec.d2_at_rank)
            hd.append(_lerp(a, b, t))
            total = total + np.float64(rec.sum)
            within += int(rec.within[0])
        out["hd_mm"][c] = max(hd)
        out["assd_mm"][c] = total / np.float64(n_p + n_g)
        out["nsd"][c] = np.float64(within) / np.float64(n_p + n_g)
    return out


def hausdorff_mean(hd: np.ndarray):
    """MONAI's do_metric_reduction(f, "mean") with get_not_nans: mean over the classes that are not NaN, then over the
    batch entries that have any -> (value, not_nans) as haus_dist_metric.aggregate() returns them"""
    f = np.asarray(hd, dtype=np.float64).copy()
    nans = np.isnan(f)
    f[nans] = 0.0
    nn = (~nans).sum(1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(nn > 0, f.sum(1) / np.maximum(nn, 1.0), 0.0)
    nb = float((nn > 0).sum())
    return (float(per.sum() / nb) if nb > 0 else 0.0), nb


def dice_from_maps(pred_u8: torch.Tensor, label: torch.Tensor, n_classes: int):
    """hard Dice of one integer label map against one label volume (any shapes with the same voxel count) from the
    confusion matrix ``bincount(pred * C + label)`` on the tensors' device -> (scores[1, C], not_nans[1, C]) with the nan
    convention of ``losses.dice_metric``: NaN where the label lacks the class.  Voxels whose prediction or label is not a
    class (an ignore value) are left out.  Not a hot path: one pass over a uint8 map per evaluated volume."""
    C = int(n_classes)
    p = pred_u8.reshape(-1).long()
    t = label.reshape(-1).long()
    assert p.numel() == t.numel(), "prediction and label differ in voxel count"
    ok = (p >= 0) & (p < C) & (t >= 0) & (t < C)
    conf = torch.bincount(p[ok] * C + t[ok], minlength=C * C).view(C, C).float()      # [pred][label]
    inter, np_, nt = conf.diagonal(), conf.sum(1), conf.sum(0)
    score = torch.where(nt > 0, 2.0 * inter / (np_ + nt), torch.full_like(inter, float("nan")))[None]
    return score, (~torch.isnan(score)).float()
