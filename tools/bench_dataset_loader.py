#!/usr/bin/env python
"""Timings of the dataset path on one MI355X (the numbers of profiles/dataset_loader_bench.txt):

    python tools/bench_dataset_loader.py > profiles/dataset_loader_bench.txt

  * msseg_aug_crop_multi against msseg_aug_crop_batch on the same single 192^3 1-channel volume, the same 8 rows of roi
    96, bf16 output: median of --iters device-timed launches after --warmup, in alternating blocks so that clock drift
    hits both alike; achieved GB/s over the bytes the gather has to move (fp32 image + uint8 label read, bf16 image +
    fp32 label written)
  * msseg_pick_voxels for a batch of 8
  * a full next(loader) of DeviceDatasetLoader (host draws, uploads, pick, gather, the one device-to-host copy), wall clock
  * the one-off preprocessing of a 512^3 int16 volume (spacing 1.5 x 0.8 x 0.8 -> 1 mm, CT window, foreground crop, pad)
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
from medicalsemseg_amd.data_device import (PICK_FG, AugRow, DeviceDatasetLoader, PickRow, VolumeDesc, _upload,  # noqa: E402
                                           preprocess_volume)
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


def stats(t):
    return f"median {np.median(t):8.2f} us   p10 {np.percentile(t, 10):8.2f}   p90 {np.percentile(t, 90):8.2f}   n {t.size}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--skip_prep", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    V, R, B = 192, 96, 8
    img = torch.randn(1, V, V, V, device=dev)
    lab = torch.zeros(V, V, V, dtype=torch.uint8, device=dev)
    lab[40:150, 30:160, 50:140] = 1
    old_rows, new_rows, picks = [], [], []
    for i in range(B):
        s = [int(rng.integers(0, V - R + 1)) for _ in range(3)]
        fl, rk, sh, sc = i % 8, i % 4, 0.05, 1.05
        old_rows.append(AugRow(*s, fl, rk, 0, sh, sc))
        new_rows.append(PickRow(0, 2, 0, 0, fl, rk, sh, sc))
        picks.append([v + R // 2 for v in s] + s + [0, 0])
    t_old, t_new = _upload(old_rows, dev), _upload(new_rows, dev)
    pk = torch.tensor(picks, dtype=torch.int32, device=dev)
    desc = _upload([VolumeDesc(img.data_ptr(), lab.data_ptr(), *img.shape)], dev)
    o_i = torch.empty(B, 1, R, R, R, dtype=torch.bfloat16, device=dev)
    o_l = torch.empty(B, 1, R, R, R, dtype=torch.float32, device=dev)
    n_i, n_l = torch.empty_like(o_i), torch.empty_like(o_l)
    f_old = lambda: hip.aug_crop_batch(img, lab, t_old, o_i, o_l, R)
    f_new = lambda: hip.aug_crop_multi(desc, 1, t_new, pk, n_i, n_l, R)
    f_old(); f_new()
    torch.cuda.synchronize()
    assert torch.equal(o_i, n_i) and torch.equal(o_l, n_l), "the two kernels disagree"
    timed(f_old, a.warmup); timed(f_new, a.warmup)
    olds, news = [], []
    for _ in range(a.blocks):
        olds.append(timed(f_old, a.iters))
        news.append(timed(f_new, a.iters))
    nbytes = B * R ** 3 * (4 + 1 + 2 + 4)
    print(f"# {torch.cuda.get_device_name(0)}; volume {V}^3 x 1 channel, {B} rows of roi {R}, bf16 image + fp32 label out; "
          f"{nbytes / 1e6:.1f} MB moved per launch; {a.blocks} alternating blocks of {a.iters} launches after {a.warmup} warm-up")
    for k, (o, n) in enumerate(zip(olds, news)):
        print(f"block {k}: aug_crop_batch {np.median(o):8.2f} us   aug_crop_multi {np.median(n):8.2f} us")
    o, n = np.concatenate(olds), np.concatenate(news)
    spread = lambda ts: (max(np.median(t) for t in ts) - min(np.median(t) for t in ts))
    print(f"msseg_aug_crop_batch (parent): {stats(o)}   {nbytes / np.median(o) / 1e3:7.1f} GB/s   block-median spread {spread(olds):.2f} us")
    print(f"msseg_aug_crop_multi (new)   : {stats(n)}   {nbytes / np.median(n) / 1e3:7.1f} GB/s   block-median spread {spread(news):.2f} us")

    # pick: 8 rows, foreground rank in the middle of a slice (a full counting scan of half a 192 x 192 slice)
    cnt = hip.slab_counts(img, lab, 0.0).cpu().numpy()
    prow = [PickRow(0, PICK_FG, 40 + 13 * i, int(cnt[40 + 13 * i, 0]) // 2, 0, 0, 0.0, 1.0) for i in range(B)]
    t_pick = _upload(prow, dev)
    out = torch.empty(B, 8, dtype=torch.int32, device=dev)
    f_pick = lambda: hip.pick_voxels(desc, 1, t_pick, B, R, 0.0, out)
    timed(f_pick, a.warmup)
    print(f"msseg_pick_voxels, batch of {B}  : {stats(timed(f_pick, a.iters))}")

    # the whole loader step over 4 cached volumes
    recs = [{"img": torch.randn(1, V, V, V, device=dev), "lab": lab.clone(), "affine": np.eye(4), "original_affine": np.eye(4),
             "filename": f"vol{k}"} for k in range(4)]
    ld = DeviceDatasetLoader(recs, R, B, a.warmup + a.iters, 2, dev, seed=1, flip_prob=0.5, rot_prob=0.5, shift_prob=0.5,
                             scale_prob=0.5, out_dtype=torch.bfloat16)
    it = iter(ld)
    for _ in range(a.warmup):
        next(it)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        t0 = time.perf_counter()
        next(it)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts = np.array(ts)
    print(f"next(DeviceDatasetLoader), wall  : {stats(ts)}   ({np.median(ts) / 3760 * 100:.1f} % of the 3.76 ms UNet step)")

    if not a.skip_prep:
        cfg = get_args(["--vol_size", "96", "--t_voxel_spacings", "--t_voxel_dims", "1.0", "1.0", "1.0", "--t_fixed_ct_intensity",
                        "--t_crop_foreground_img", "--t_spatial_pad"])
        big = rng.integers(-1024, 1500, (1, 512, 512, 512), dtype=np.int16)
        big[:, :20] = -1024
        blab = np.zeros((512, 512, 512), dtype=np.uint8)
        blab[100:300, 100:300, 100:300] = 1
        aff = np.diag([1.5, 0.8, 0.8, 1.0])
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = preprocess_volume(big, blab, aff, cfg, dev)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            shape = tuple(rec["img"].shape)
            del rec
        print(f"preprocess_volume, 512^3 int16 (upload + orientation + spacing + window + crop): {min(ts) * 1e3:.1f} ms best of 3 "
              f"({', '.join(f'{t * 1e3:.1f}' for t in ts)}), cached shape {shape}")


if __name__ == "__main__":
    main()
