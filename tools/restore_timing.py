"""Times of hip.restore_native_u8 (csrc/restore.hip) at a native grid of SIZE^3: three orientations (identity, all three
axes flipped, the fastest axis permuted: perm (2, 1, 0)), without and with a (1.5, 1.5, 1.5) spacing scale, in nearest mode
and in linear mode with C = 3 and C = 14.  WARMUP calls, then REPEATS times a device-event pair around INNER back-to-back
calls; a row is the median (min - max) of the per-call times of the repeats, the effective GB/s against the kernel's own
minimum traffic (the model-grid source read once + one byte per native voxel written) and the time relative to the
identity orientation of the same mode, C and scale.  Printed as a markdown table.
usage: python tools/restore_timing.py [--size 512]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from medicalsemseg_amd import hip

WARMUP, REPEATS, INNER = 2, 7, 5
ORIENTATIONS = [("identity", (0, 1, 2), (0, 0, 0)), ("flips only", (0, 1, 2), (1, 1, 1)), ("perm (2, 1, 0)", (2, 1, 0), (0, 0, 0))]
dev = torch.device("cuda:0")


def descriptor(n, perm, flip, scale):
    d = hip.RestoreDesc()
    for k in range(3):
        g = max(int(np.round((n - 1) * scale + 1.0)), 1)
        d.native[k], d.perm[k], d.flip[k], d.grid[k], d.offset[k], d.model[k], d.scale[k] = n, perm[k], flip[k], g, 0, g, scale
    return d


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / INNER)
    ts.sort()
    return ts[REPEATS // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    n = args.size
    print(f"native {n}^3; {WARMUP} warm-up calls, median (min - max) over {REPEATS} repeats of {INNER} calls each", flush=True)
    print("| mode | scale | orientation | ms per call | GB/s of minimum traffic | of identity |\n|---|---|---|---|---|---|")
    g = torch.Generator(device=dev).manual_seed(0)
    for scale in (1.0, 1.5):
        m = max(int(np.round((n - 1) * scale + 1.0)), 1)
        logits = torch.randn(14, m, m, m, device=dev, generator=g)
        labels = hip.argmax_u8(logits[:3].contiguous())
        for mode, C in (("nearest", 0), ("linear", 3), ("linear", 14)):
            src = labels if mode == "nearest" else logits[:C]
            nbytes = src.numel() * src.element_size() + n ** 3
            base = None
            for name, perm, flip in ORIENTATIONS:
                d = descriptor(n, perm, flip, scale)
                med, lo, hi = timed(lambda: hip.restore_native_u8(src, d, mode))
                base = med if base is None else base
                print(f"| {mode}{'' if not C else f' C = {C}'} | {scale:g} | {name} | {med:.3f} ({lo:.3f} - {hi:.3f}) | "
                      f"{nbytes / med * 1e-6:.0f} | {med / base:.2f} |", flush=True)
        del logits, labels


if __name__ == "__main__":
    main()
