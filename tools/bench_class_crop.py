#!/usr/bin/env python
"""Cost of the class-ratio crop centres on one MI355X (the numbers of profiles/class_crop_bench.txt and DESIGN.md section 9):

    python tools/bench_class_crop.py > profiles/class_crop_bench.txt

  * msseg_class_candidate_mask on a 4 x 240 x 240 x 155 volume (a BraTS case) with labels 0..3, dilation 48, three classes,
    and the per-slice counts from the label and from the mask: median of --iters device-timed calls after --warmup
  * per-batch assembly (the pick launch + the gather launch, device time between two events around both) of
    DeviceDatasetLoader over --volumes such volumes, batch --batch, roi --roi: crop="fgbg", crop="class_ratios" without a
    dilation and with dilation 48; every mode is measured --repeats times so that its own run-to-run spread shows
  * --fgbg_only measures the fgbg loader alone and uses nothing this crop added, so the same script also runs on an older
    checkout of the package (put it first on PYTHONPATH)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.exists(os.path.join(p, "medicalsemseg_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

from medicalsemseg_amd import hip  # noqa: E402
from medicalsemseg_amd.data_device import DeviceDatasetLoader  # noqa: E402


def timed(fn, iters):
    """device time of every call, microseconds"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in ev])


def brats_like(shape, seed):
    """four modalities inside an ellipsoid (zeros outside, as a skull-stripped case), nested tumour labels 1..3 near a
    seed-dependent point: the classes fill ~2 %, ~1 % and ~0.3 % of the grid"""
    rng = np.random.default_rng(seed)
    ax = [np.linspace(-1, 1, s, dtype=np.float32) for s in shape[1:]]
    r = (ax[0][:, None, None] / 0.9) ** 2 + (ax[1][None, :, None] / 0.85) ** 2 + (ax[2][None, None, :] / 0.95) ** 2
    img = np.zeros(shape, np.float32)
    for c in range(shape[0]):
        v = rng.standard_normal(shape[1:], dtype=np.float32) + np.float32(0.3 * c)
        img[c] = np.where(r < 1.0, np.where(v == 0, np.float32(1e-3), v), np.float32(0.0))
    o = rng.uniform(-0.3, 0.3, 3).astype(np.float32)
    t = (ax[0][:, None, None] - o[0]) ** 2 + (ax[1][None, :, None] - o[1]) ** 2 + (ax[2][None, None, :] - o[2]) ** 2
    lab = np.zeros(shape[1:], np.uint8)
    for k, rad in ((2, 0.34), (1, 0.27), (3, 0.18)):
        lab[t < rad * rad] = k
    return img, lab


def loader_stats(make, n_batches, warmup, repeats):
    """per-batch device time (pick + gather) of `repeats` fresh loaders: the median of each run, microseconds"""
    meds = []
    for rep in range(repeats):
        ld = make(rep)
        it = iter(ld)
        ts = []
        for k in range(n_batches + warmup):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            batch = next(it)
            b.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ts.append(a.elapsed_time(b) * 1e3)
            del batch
        meds.append(float(np.median(ts)))
    return meds


def entry_point_split(make, n_batches, warmup):
    """device time per entry point (hip.TIMER: an event pair around every library call), microseconds per batch"""
    it = iter(make(0))
    for _ in range(warmup):
        next(it)
    torch.cuda.synchronize()
    hip.TIMER.records.clear()
    hip.TIMER.enabled = True
    try:
        for _ in range(n_batches):
            next(it)
        torch.cuda.synchronize()
    finally:
        hip.TIMER.enabled = False
    out = {k: v["total_ms"] * 1e3 / n_batches for k, v in hip.TIMER.summary().items()}
    hip.TIMER.records.clear()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=4, default=[4, 240, 240, 155])
    ap.add_argument("--volumes", type=int, default=4)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--roi", type=int, default=96)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dilation", type=int, default=48)
    ap.add_argument("--fgbg_only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = tuple(a.shape)
    recs = []
    for k in range(a.volumes):
        img, lab = brats_like(shape, k)
        recs.append({"img": torch.from_numpy(img).to(dev), "lab": torch.from_numpy(lab).to(dev), "affine": np.eye(4),
                     "original_affine": np.eye(4), "filename": f"case{k}"})
    vox = int(np.prod(shape[1:]))
    lab0, img0 = recs[0]["lab"], recs[0]["img"][0]
    share = ", ".join("{:.2f} %".format(float((lab0 == c).float().mean()) * 100) for c in range(4))
    print(f"# {torch.cuda.get_device_name(0)}; {a.volumes} volume(s) {shape} fp32 + uint8 labels 0..3 ({share} of volume 0), "
          f"{float((img0 != 0).float().mean()) * 100:.1f} % non-zero; package {os.path.relpath(os.path.dirname(hip.__file__), ROOT)}")
    common = dict(patches_per_image=1, device=dev, image_threshold=0.0, image_rule="ne", flip_prob=0.5, rot_prob=0.5,
                  shift_prob=0.5, scale_prob=0.5)
    modes = [("fgbg (pos 1 : neg 1)", lambda s: DeviceDatasetLoader(recs, a.roi, a.batch, 10 ** 6, seed=s, crop="fgbg", **common))]
    if not a.fgbg_only:
        img, lab = recs[0]["img"], recs[0]["lab"]
        calls = [(f"msseg_class_candidate_mask, N = {a.dilation}, classes 1 2 3",
                  lambda: hip.class_candidate_mask(img, lab, (1, 2, 3), a.dilation, 0.0, "ne")),
                 ("msseg_class_candidate_mask, N = 1, classes 1 2 3", lambda: hip.class_candidate_mask(img, lab, (1, 2, 3), 1, 0.0, "ne")),
                 ("msseg_class_slab_counts from the label, K = 4", lambda: hip.class_slab_counts(img, lab, 4, 0.0, "ne"))]
        mask = hip.class_candidate_mask(img, lab, (1, 2, 3), a.dilation, 0.0, "ne")
        calls.append(("msseg_class_slab_counts from the mask, K = 4", lambda: hip.class_slab_counts(img, lab, 4, 0.0, "ne", mask=mask)))
        calls.append(("msseg_slab_counts (fg / bg)", lambda: hip.slab_counts(img, lab, 0.0, "ne")))
        print(f"# one volume = {vox / 1e6:.2f} M voxels; median of {a.iters} device-timed calls after {a.warmup} warm-up "
              f"(the mask call includes its two torch.empty allocations)")
        for name, fn in calls:
            timed(fn, a.warmup)
            t = timed(fn, a.iters)
            print(f"{name:58s}: median {np.median(t):9.1f} us   p10 {np.percentile(t, 10):9.1f}   p90 {np.percentile(t, 90):9.1f}")
        cnt = hip.class_slab_counts(img, lab, 4, 0.0, "ne", mask=mask).sum(0).tolist()
        cnt0 = hip.class_slab_counts(img, lab, 4, 0.0, "ne").sum(0).tolist()
        print(f"candidates of volume 0 with N = {a.dilation}: {cnt}; with N = 0: {cnt0}")
        ratios = (0.2, 1.0, 1.0, 1.0)
        t0 = time.perf_counter()
        ld = DeviceDatasetLoader(recs, a.roi, a.batch, 1, seed=0, crop="class_ratios", class_ratios=ratios,
                                 center_dilation=a.dilation, **common)
        torch.cuda.synchronize()
        print(f"DeviceDatasetLoader construction with N = {a.dilation}: {(time.perf_counter() - t0) * 1e3:.1f} ms wall clock for "
              f"{a.volumes} volumes (masks + counts + read-back), masks hold {sum(m.numel() * 2 for m in ld.masks) / 1e6:.1f} MB")
        del ld
        modes += [("class_ratios 0.2 1 1 1, N = 0", lambda s: DeviceDatasetLoader(recs, a.roi, a.batch, 10 ** 6, seed=s,
                                                                                  crop="class_ratios", class_ratios=ratios, **common)),
                  (f"class_ratios 0.2 1 1 1, N = {a.dilation}",
                   lambda s: DeviceDatasetLoader(recs, a.roi, a.batch, 10 ** 6, seed=s, crop="class_ratios", class_ratios=ratios,
                                                 center_dilation=a.dilation, **common))]
    print(f"# per-batch assembly, batch {a.batch} x {shape[0]} x {a.roi}^3 fp32: device time from before the pick to after the "
          f"gather (host draws and the row upload in between included), median of {a.batches} batches after {a.warmup}, "
          f"{a.repeats} runs with seeds 0..{a.repeats - 1}")
    for name, make in modes:
        meds = loader_stats(make, a.batches, a.warmup, a.repeats)
        print(f"{name:34s}: medians {', '.join(f'{m:7.1f}' for m in meds)} us   median of runs {np.median(meds):7.1f}   "
              f"spread (max - min) {max(meds) - min(meds):6.1f}")
    print(f"# the same per entry point: device time between an event pair around each library call, mean over {a.batches} batches")
    for name, make in modes:
        split = entry_point_split(make, a.batches, a.warmup)
        print(f"{name:34s}: " + ", ".join(f"{k} {v:6.1f} us" for k, v in sorted(split.items())))


if __name__ == "__main__":
    main()
