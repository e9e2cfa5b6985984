"""Cost of mirror test-time augmentation (sliding_window_inference(..., mirror_axes=...)) on the sliding-window workload of
bench.py: the UNet in bf16 / eval, a seeded SIZE^3 volume, roi 96^3, overlap 0.5, gaussian, 8 rows per replayed forward.
WARMUP calls, then the median / min / max of RUNS calls (host clock around a device synchronise) of
  M = 1, 2, 4, 8   mirror_axes = (), (2,), (1, 2), (0, 1, 2): the masks are rows of the window table
  flip loop, M = 8  the same eight predictions written around the call: torch.flip of the volume, a plain call, torch.flip of
                    its logits, the mean of the eight results
all in the same process on the same volume, printed as a markdown table with each row's time over M x the M = 1 time.  The flip
loop slides its windows over the flipped volume (the clamped last start falls on the other side) and normalises each pass on its
own, so its result is close to, not equal to, the fused one; the largest difference is printed.
usage: python tools/bench_sw_mirror.py [--size 512] [--roi 96] [--sw_batch 8] [--runs 3]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from medicalsemseg_amd.engine.utils import mirror_masks, sliding_window_inference
from medicalsemseg_amd.models.unet import UNet

WARMUP = 1
dev = torch.device("cuda:0")


def timed(fn, runs):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--roi", type=int, default=96)
    ap.add_argument("--sw_batch", type=int, default=8)
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    torch.manual_seed(0)
    net = UNet(1, args.classes, compute_dtype=torch.bfloat16).to(dev).eval()
    vol = torch.randn(1, 1, args.size, args.size, args.size, generator=torch.Generator().manual_seed(13)).to(dev)
    aff = torch.ones(1, 3, device=dev)

    def infer(v, axes=()):
        with torch.no_grad():
            return sliding_window_inference(v, aff, (args.roi,) * 3, args.sw_batch, net, overlap=0.5, mode="gaussian",
                                            mirror_axes=axes)

    def flip_loop(axes=(0, 1, 2)):
        acc = None
        for m in mirror_masks(axes):
            dims = [2 + a for a in range(3) if m >> a & 1]
            y = infer(torch.flip(vol, dims) if dims else vol)
            y = torch.flip(y, dims) if dims else y
            acc = y if acc is None else acc.add_(y)
        return acc.div_(len(mirror_masks(axes)))

    rows = [("M = 1, `mirror_axes=()`", 1, lambda: infer(vol)),
            ("M = 2, `mirror_axes=(2,)`", 2, lambda: infer(vol, (2,))),
            ("M = 4, `mirror_axes=(1, 2)`", 4, lambda: infer(vol, (1, 2))),
            ("M = 8, `mirror_axes=(0, 1, 2)`", 8, lambda: infer(vol, (0, 1, 2))),
            ("M = 8, `torch.flip` loop around the plain call", 8, flip_loop)]
    print(f"{args.size}^3, roi {args.roi}^3, overlap 0.5, {args.sw_batch} rows per forward, {args.classes} classes, bf16; "
          f"{WARMUP} warm-up + {args.runs} timed calls per row", flush=True)
    print("| call | median ms (min – max) | over M x (M = 1) |\n|---|---|---|")
    base = None
    for name, m, fn in rows:
        med, lo, hi = timed(fn, args.runs)
        base = med if base is None else base
        print(f"| {name} | {med:.1f} ({lo:.1f} – {hi:.1f}) | {med / (m * base):.3f} |", flush=True)
    fused, loop = infer(vol, (0, 1, 2)), flip_loop()
    print(f"max |fused - flip loop| = {float((fused - loop).abs().max()):.3e} at max |logit| = {float(fused.abs().max()):.3e}",
          flush=True)


if __name__ == "__main__":
    main()
