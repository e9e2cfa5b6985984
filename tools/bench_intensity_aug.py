#!/usr/bin/env python
"""Cost of the intensity augmentation on one MI355X (the numbers of DESIGN.md section 9):

    python tools/bench_intensity_aug.py > profiles/intensity_aug_bench.txt

  * a full next(loader) of DeviceDatasetLoader at roi 96, batch 2, one channel, bf16 out, wall clock including the final
    synchronisation: every intensity stage at probability 1 against every stage off (the parent's path), in alternating
    blocks so that clock drift hits both alike
  * device time of msseg_intensity_aug alone on a fixed batch and table, for growing prefixes of the chain: the difference
    between two lines is the cost of the passes the longer one adds
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from medicalsemseg_amd import hip  # noqa: E402
from medicalsemseg_amd.data_device import DeviceDatasetLoader, IntensityRow, intensity_config  # noqa: E402


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


def wall(loader_iter, n):
    t = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        next(loader_iter)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--roi", type=int, default=96)
    ap.add_argument("--batch", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    R, B = a.roi, a.batch
    g = torch.Generator(device=dev).manual_seed(0)
    recs = []
    for k in range(4):
        img = torch.randn(1, 160, 192, 176, device=dev, generator=g)
        lab = (torch.rand(160, 192, 176, device=dev, generator=g) < 0.1).to(torch.uint8)
        recs.append({"img": img, "lab": lab, "affine": np.eye(4), "original_affine": np.eye(4), "filename": f"v{k}"})
    on = intensity_config(noise_prob=1.0, blur_prob=1.0, blur_channel_prob=1.0, contrast_prob=1.0, gamma_invert_prob=1.0,
                          gamma_prob=1.0)
    total = (a.iters + a.warmup) * a.blocks
    kw = dict(patches_per_image=1, device=dev, seed=1, flip_prob=0.5, rot_prob=0.5, shift_prob=0.5, scale_prob=0.5,
              out_dtype=torch.bfloat16)
    its = {"every stage off": iter(DeviceDatasetLoader(recs, R, B, total, **kw)),
           "every stage at probability 1": iter(DeviceDatasetLoader(recs, R, B, total, intensity=on, **kw))}
    times = {k: [] for k in its}
    for _ in range(a.blocks):
        for k, it in its.items():
            wall(it, a.warmup)
            times[k] += wall(it, a.iters)
    print(f"next(DeviceDatasetLoader), roi {R}, batch {B}, 1 channel, bf16 out, wall clock with the final synchronisation")
    for k, t in times.items():
        print(f"  {k:32s} {stats(np.array(t))}")

    print(f"msseg_intensity_aug alone, [{B}, 1, {R}, {R}, {R}] fp32 -> bf16, device time")
    x = torch.randn(B, 1, R, R, R, device=dev, generator=g)
    out = torch.empty_like(x, dtype=torch.bfloat16)
    chains = [("copy (no bit set)", 0, 1.0), ("noise", 1, 1.0), ("blur sigma 1.0 (radius 4)", 2, 1.0), ("noise + blur sigma 1.0", 3, 1.0),
              ("noise + blur + contrast", 7, 1.0), ("... + gamma inverted", 15, 1.0), ("full chain", 31, 1.0),
              ("full chain, blur sigma 0.5 (radius 2)", 31, 0.5), ("full chain, blur sigma 2.0 (radius 8)", 31, 2.0)]
    for name, mask, sigma in chains:
        rows = (IntensityRow * B)(*[IntensityRow(mask, 0.1, 1234567 + j, sigma, 1.2, 0.8, 1.3) for j in range(B)])
        # the C entry point with a table uploaded once: the binding's upload would sit inside the timed interval
        table = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
        nws = int(hip.lib().msseg_intensity_aug_workspace_bytes(B, 1, R, R, R))
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def fn():
            rc = hip.lib().msseg_intensity_aug(x.data_ptr(), ctypes.addressof(rows), table.data_ptr(), B, 1, R, R, R,
                                               out.data_ptr(), hip.BF16, ws.data_ptr(), nws, stream)
            assert rc == 0, hip.lib().msseg_last_error()
        timed(fn, a.warmup)
        print(f"  {name:40s} {stats(timed(fn, a.iters))}")


if __name__ == "__main__":
    main()
