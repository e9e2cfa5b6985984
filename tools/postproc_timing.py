"""Times of the post-processing calls (csrc/components.hip) between device events on a seeded synthetic three-class map: two
large blobs (a class 1 ball and a class 2 ball), a few thousand 3^3 specks of both classes in the background and a few
thousand 3^3 cavities of class 0 inside the balls.  WARMUP calls, then the median / min / max of RUNS calls of
  1  hip.keep_largest_u8
  2  hip.postprocess_u8(min_size=64)
  3  hip.postprocess_u8(min_size=64, keep_largest=True)
  4  hip.postprocess_u8(fill_holes=True)
  5  hip.postprocess_u8(min_size=64, keep_largest=True, fill_holes=True)
all in the same process on the same input, printed as a markdown table with the per-class stats of row 5.  --scipy also runs
the scipy equivalent of row 5 once on the host (ndimage.label + bincount per class, then binary_fill_holes per class).
--rows 4 times only the listed rows (for a kernel trace of one call's passes in a run of its own).
usage: python tools/postproc_timing.py [--scipy] [--size 512] [--connectivity 26] [--hole_connectivity 26] [--rows 1,2,3,4,5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from medicalsemseg_amd import hip

WARMUP, RUNS = 5, 25
N_CLASSES = 3
dev = torch.device("cuda:0")


def blobs_specks_cavities(n: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(seed)
    ax = torch.arange(n, device=dev, dtype=torch.float32)

    def ball(cz, cy, cx, r):
        return (ax.view(n, 1, 1) - cz * n) ** 2 + (ax.view(1, n, 1) - cy * n) ** 2 + (ax.view(1, 1, n) - cx * n) ** 2 <= (r * n) ** 2

    lab = torch.zeros(n, n, n, dtype=torch.uint8, device=dev)
    lab[ball(0.35, 0.40, 0.35, 0.25)] = 1
    lab[ball(0.70, 0.65, 0.70, 0.20)] = 2
    near = F.max_pool3d((lab > 0)[None, None].half(), 9, 1, 4)[0, 0] > 0          # the balls and four voxels around them
    core = F.max_pool3d((lab == 0)[None, None].half(), 9, 1, 4)[0, 0] == 0        # at least four voxels inside a ball
    u = torch.rand(n, n, n, device=dev, generator=g)

    def cubes(seeds):                                                             # 3^3 voxels around every seed
        return F.max_pool3d(seeds[None, None].half(), 3, 1, 1)[0, 0] > 0

    p = 3000.0 / n ** 3
    lab[cubes(~near & (u < p))] = 1
    lab[cubes(~near & (u > 1.0 - p))] = 2
    lab[cubes(core & (u < 4000.0 / max(int(core.sum()), 1)))] = 0
    return lab.contiguous()


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[RUNS // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scipy", action="store_true", help="also run the scipy equivalent of all three steps on the host, once")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--connectivity", type=int, default=26)
    ap.add_argument("--hole_connectivity", type=int, default=26)
    ap.add_argument("--rows", default="1,2,3,4,5", help="the rows to time; 'of row 1' refers to the first one timed")
    args = ap.parse_args()
    lab = blobs_specks_cavities(args.size)
    out = torch.empty_like(lab)
    conn, hole = args.connectivity, args.hole_connectivity
    pp = lambda **kw: hip.postprocess_u8(lab, N_CLASSES, connectivity=conn, hole_connectivity=hole, out=out, **kw)   # noqa: E731
    rows = [
        ("1 `keep_largest_u8`", lambda: hip.keep_largest_u8(lab, N_CLASSES, conn, out=out)),
        ("2 `postprocess_u8(min_size=64)`", lambda: pp(min_size=64)),
        ("3 `postprocess_u8(min_size=64, keep_largest=True)`", lambda: pp(min_size=64, keep_largest=True)),
        ("4 `postprocess_u8(fill_holes=True)`", lambda: pp(fill_holes=True)),
        ("5 all three steps", lambda: pp(min_size=64, keep_largest=True, fill_holes=True)),
    ]
    print(f"{args.size}^3, {N_CLASSES} classes, connectivity {conn}, hole connectivity {hole}; voxels per class "
          f"{torch.bincount(lab.reshape(-1).long(), minlength=N_CLASSES).tolist()}", flush=True)
    print("| call | median ms (min – max) | of row 1 |\n|---|---|---|")
    base = None
    for name, fn in [r for r in rows if r[0][0] in args.rows.split(",")]:
        med, lo, hi = timed(fn)
        base = med if base is None else base
        print(f"| {name} | {med:.3f} ({lo:.3f} – {hi:.3f}) | {med / base:.2f} |", flush=True)
    _, stats = hip.postprocess_u8(lab, N_CLASSES, min_size=64, keep_largest=True, connectivity=conn, fill_holes=True,
                                  hole_connectivity=hole, return_stats=True)
    print("stats of row 5 {components, small removed, voxels in them, removed by keep-largest, filled, final}:",
          stats.cpu().tolist(), flush=True)
    if args.scipy:
        from scipy import ndimage
        a = lab.cpu().numpy()
        t0 = time.perf_counter()
        st = ndimage.generate_binary_structure(3, 1 if conn == 6 else 3)
        res = a.copy()
        for c in range(1, N_CLASSES):
            cc, k = ndimage.label(a == c, structure=st)
            sizes = np.bincount(cc.ravel(), minlength=k + 1)
            sizes[0] = 0
            keep = int(np.argmax(sizes)) if sizes.max() >= 64 else -1
            res[(a == c) & (cc != keep)] = 0
        t1 = time.perf_counter()
        print(f"scipy label + bincount + mask, {N_CLASSES - 1} classes: {t1 - t0:.2f} s (one run on the host)", flush=True)
        st = ndimage.generate_binary_structure(3, 1 if hole == 6 else 3)
        for c in range(1, N_CLASSES):
            res[ndimage.binary_fill_holes(res == c, structure=st)] = c
        t2 = time.perf_counter()
        print(f"scipy binary_fill_holes, {N_CLASSES - 1} classes: {t2 - t1:.2f} s (one run on the host)", flush=True)
        same = bool((torch.from_numpy(res).to(dev) == hip.postprocess_u8(
            lab, N_CLASSES, min_size=64, keep_largest=True, connectivity=conn, fill_holes=True, hole_connectivity=hole)).all())
        print(f"device map == scipy map: {same}", flush=True)


if __name__ == "__main__":
    main()
