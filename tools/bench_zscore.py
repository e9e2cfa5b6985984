#!/usr/bin/env python
"""Cost of --t_zscore / --t_zscore_clip on one MI355X (the numbers of profiles/zscore_bench.txt and DESIGN.md section 9):

    python tools/bench_zscore.py > profiles/zscore_bench.txt

  * the three entry points of csrc/volume_stats.hip on a skull-stripped 4 x 240 x 240 x 155 fp32 volume (a BraTS case):
    median of --iters device-timed calls after --warmup; achieved GB/s over the bytes each has to move (the volume read
    once per pass: 4 for the select, 2 for the moments, 1 read + 1 write for the apply)
  * preprocess_volume on that volume (upload, foreground box, crop + pad, and with the flags the z-score and its one
    read-back) with and without --t_zscore --t_zscore_clip 0.5 99.5, wall clock around a device synchronise
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from medicalsemseg_amd import hip  # noqa: E402
from medicalsemseg_amd.data_device import preprocess_volume  # noqa: E402
from medicalsemseg_amd.utils.arguments import get_args  # noqa: E402


def timed(fn, iters):
    """device time of every call, microseconds"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in ev])


def mr_volume(shape, seed=0):
    """four modalities on different scales inside an ellipsoid that fills ~40 % of the grid, zeros outside"""
    rng = np.random.default_rng(seed)
    ax = [np.linspace(-1, 1, s, dtype=np.float32) for s in shape[1:]]
    r = (ax[0][:, None, None] / 0.9) ** 2 + (ax[1][None, :, None] / 0.85) ** 2 + (ax[2][None, None, :] / 0.95) ** 2
    img = np.zeros(shape, np.float32)
    for c in range(shape[0]):
        v = (300.0 * (c + 1) + 90.0 * (c + 1) * rng.standard_normal(shape[1:], dtype=np.float32)).astype(np.float32)
        img[c] = np.where(r < 1.0, np.maximum(v, 1.0), 0.0)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=4, default=[4, 240, 240, 155])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shape = tuple(a.shape)
    img = mr_volume(shape)
    x = torch.from_numpy(img).to(dev)
    nbytes = x.numel() * 4
    scratch = hip._stats_scratch(x)
    sel = hip.select_f32(x, percentages=(0.5, 99.5), scratch=scratch)
    stats = hip.masked_moments(x, sel[:, 5:7], scratch=scratch)
    work = x.clone()
    calls = [("msseg_select_f32 (2 percentiles)", 4, lambda: hip.select_f32(x, percentages=(0.5, 99.5), scratch=scratch)),
             ("msseg_masked_moments (clipped)", 2, lambda: hip.masked_moments(x, sel[:, 5:7], scratch=scratch)),
             ("msseg_masked_moments (no clip)", 2, lambda: hip.masked_moments(x, None, scratch=scratch)),
             ("msseg_zscore_apply", 2, lambda: hip.zscore_apply_(work, stats))]
    print(f"# {torch.cuda.get_device_name(0)}; volume {shape} fp32 = {nbytes / 1e6:.1f} MB, "
          f"{float((x != 0).float().mean()) * 100:.1f} % non-zero; median of {a.iters} device-timed calls after {a.warmup} warm-up")
    total = 0.0
    for name, passes, fn in calls:
        timed(fn, a.warmup)
        t = timed(fn, a.iters)
        med = float(np.median(t))
        total += med if "no clip" not in name else 0.0
        print(f"{name:36s}: median {med:9.1f} us   p10 {np.percentile(t, 10):9.1f}   p90 {np.percentile(t, 90):9.1f}   "
              f"{passes} pass(es) = {passes * nbytes / 1e6:7.1f} MB   {passes * nbytes / med / 1e3:7.1f} GB/s")
    print(f"select + clipped moments + apply    : {total:9.1f} us device time, {8 * nbytes / 1e6:.1f} MB")

    flags = ["--vol_size", "96", "--in_chans", str(shape[0]), "--t_crop_foreground_img", "--t_spatial_pad"]
    for label, extra in (("without --t_zscore", []), ("--t_zscore", ["--t_zscore"]),
                         ("--t_zscore --t_zscore_clip 0.5 99.5", ["--t_zscore", "--t_zscore_clip", "0.5", "99.5"])):
        cfg = get_args(flags + extra)
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = preprocess_volume(img, None, np.eye(4), cfg, dev)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            cached = tuple(rec["img"].shape)
            del rec
        print(f"preprocess_volume, {label:36s}: {min(ts[1:]) * 1e3:7.2f} ms best of 4 after one warm-up "
              f"({', '.join(f'{t * 1e3:.2f}' for t in ts)}), cached shape {cached}")


if __name__ == "__main__":
    main()
