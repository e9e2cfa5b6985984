"""Time of hip.keep_largest_u8 (csrc/components.hip: six kernels and one memset per call) between device events: WARMUP calls,
then the median / min / max of RUNS calls, for both connectivities, on
  * a seeded 512^3 three-class map: nested spheres (class 1 shell around a class 2 core) plus Bernoulli islands of both
    classes -- what an arg-max map of an organ with a lesion looks like, with the stray voxels the step removes;
  * the 96 x 128 x 160 thresholded smoothed-noise map of tests/test_gpu_components.py (hundreds of components per class).
Bytes: the passes' algorithmic traffic per voxel -- tile 1 + 8, count 8 + 4, select 4, filter 5 + 1 = 31 B (the border pass
touches tile faces only and is left out) -- over the time, against the 8 TB/s HBM peak.  --scipy also times the scipy
restatement (ndimage.label + bincount per class) of the 512^3 map on the host, one run.
usage: python tools/bench_components.py [--scipy] [--size 512]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from medicalsemseg_amd import hip

WARMUP, RUNS = 5, 25
BYTES_PER_VOXEL = 31
HBM_PEAK = 8.0e12
dev = torch.device("cuda:0")


def spheres_with_islands(n: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(seed)
    ax = torch.arange(n, device=dev, dtype=torch.float32) - (n - 1) / 2
    r2 = ax.view(n, 1, 1) ** 2 + ax.view(1, n, 1) ** 2 + ax.view(1, 1, n) ** 2
    lab = torch.zeros(n, n, n, dtype=torch.uint8, device=dev)
    lab[r2 <= (0.30 * n) ** 2] = 1
    lab[r2 <= (0.12 * n) ** 2] = 2
    u = torch.rand(n, n, n, device=dev, generator=g)
    outside = r2 > (0.33 * n) ** 2
    lab[outside & (u < 0.01)] = 1
    lab[outside & (u > 0.99)] = 2
    return lab.contiguous()


def blobs() -> torch.Tensor:
    from scipy import ndimage
    v = ndimage.gaussian_filter(np.random.default_rng(1).standard_normal((96, 128, 160)).astype(np.float32), 2.0)
    lab = np.zeros(v.shape, np.uint8)
    lab[v > 0.06] = 1
    lab[v < -0.06] = 2
    return torch.from_numpy(lab).to(dev)


def time_case(name: str, lab: torch.Tensor, n_classes: int):
    out = torch.empty_like(lab)
    for conn in (6, 26):
        for _ in range(WARMUP):
            _, stats = hip.keep_largest_u8(lab, n_classes, conn, out=out, return_stats=True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(RUNS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip.keep_largest_u8(lab, n_classes, conn, out=out)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        med = ts[RUNS // 2]
        nbytes = lab.numel() * BYTES_PER_VOXEL
        print(f"{name} connectivity {conn}: median {med:.3f} ms, min {ts[0]:.3f}, max {ts[-1]:.3f} over {RUNS} calls; "
              f"{nbytes / 1e6:.0f} MB algorithmic -> {nbytes / (med * 1e-3) / 1e12:.2f} TB/s = "
              f"{100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of HBM peak; stats {stats.cpu().tolist()}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scipy", action="store_true", help="also time the scipy restatement of the large map on the host")
    ap.add_argument("--size", type=int, default=512)
    args = ap.parse_args()
    big = spheres_with_islands(args.size)
    time_case(f"{args.size}^3 spheres + islands, 3 classes", big, 3)
    time_case("96x128x160 blobs, 3 classes", blobs(), 3)
    if args.scipy:
        from scipy import ndimage
        a = big.cpu().numpy()
        for conn in (6, 26):
            st = ndimage.generate_binary_structure(3, 1 if conn == 6 else 3)
            t0 = time.perf_counter()
            for c in (1, 2):
                cc, n = ndimage.label(a == c, structure=st)
                if n:
                    k = int(np.argmax(np.bincount(cc.ravel())[1:])) + 1
                    _ = (a == c) & (cc != k)          # the voxels the filter would clear
            print(f"scipy label + bincount, 2 classes, {args.size}^3, connectivity {conn}: {time.perf_counter() - t0:.2f} s "
                  f"(one run on the host)", flush=True)


if __name__ == "__main__":
    main()
