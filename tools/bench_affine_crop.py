"""Timing of the affine crop gather (msseg_aug_crop_affine, csrc/dataprep.hip) next to the plain gather it extends
(msseg_aug_crop_multi): batch 2 of 96^3 patches drawn from two cached volumes of 160 x 192 x 176, C = 1 and 4, fp32 and bf16
output; the affine kernel with identity matrices (every fraction 0: the same voxels as the plain gather, through 8 taps) and
with random rotations of +-30 degrees per axis and zooms of 0.7-1.4.  The three launches alternate sample by sample in one
process; device events, warm-up, a timed window of at least one second per figure.  Columns: us per call, the ratio to the
plain gather and the share of a 3.76 ms UNet training step.
usage: python tools/bench_affine_crop.py [min_seconds]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from medicalsemseg_amd import hip
from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow, VolumeDesc, _upload, affine_matrix

WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
STEP_US = 3760.0
SHAPE, ROI, BATCH = (160, 192, 176), 96, 2
dev = torch.device("cuda:0")


def sample(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def alternate(fns):
    """us per call of every function, samples of about 5 ms alternating until each has WINDOW seconds on the device"""
    reps = []
    for f in fns:
        f()
        torch.cuda.synchronize()
        t = sample(f, 1)                       # second call: warm
        reps.append(max(1, min(1000, int(5e-3 / max(t, 1e-6)))))
    tot, cnt = [0.0] * len(fns), [0] * len(fns)
    t0 = time.time()
    while any(t < WINDOW for t in tot) and time.time() - t0 < 60:
        for i, f in enumerate(fns):
            if tot[i] < WINDOW:
                tot[i] += sample(f, reps[i])
                cnt[i] += reps[i]
    return [tot[i] / cnt[i] * 1e6 for i in range(len(fns))]


rng = np.random.default_rng(5)
print("  C  dtype |  crop_multi   affine identity (ratio, % of step)   affine +-30 deg / 0.7-1.4 (ratio, % of step)   (us per call)")
for chans in (1, 4):
    vols = [(torch.randn(chans, *SHAPE, device=dev), torch.randint(0, 3, SHAPE, device=dev, dtype=torch.uint8)) for _ in range(2)]
    desc = _upload([VolumeDesc(i.data_ptr(), l.data_ptr(), *i.shape) for i, l in vols], dev)
    rows, picks, mats = [], [], []
    for j in range(BATCH):
        start = [int(rng.integers(0, n - ROI + 1)) for n in SHAPE]
        rows.append(PickRow(j % 2, PICK_VOXEL, 0, 0, int(rng.integers(0, 8)), int(rng.integers(0, 4)), 0.05, 1.1))
        picks.append([s + ROI // 2 for s in start] + start + [0, 0])
        mats.append(affine_matrix(np.deg2rad(rng.uniform(-30.0, 30.0, 3)), float(rng.uniform(0.7, 1.4))))
    table, pk = _upload(rows, dev), torch.tensor(picks, dtype=torch.int32, device=dev)
    eye = torch.from_numpy(np.tile(np.eye(3), (BATCH, 1, 1))).to(dev)
    rnd = torch.from_numpy(np.stack(mats)).to(dev)
    for dtype in (torch.float32, torch.bfloat16):
        img = torch.empty(BATCH, chans, ROI, ROI, ROI, dtype=dtype, device=dev)
        lab = torch.empty(BATCH, 1, ROI, ROI, ROI, dtype=torch.float32, device=dev)
        ref = torch.empty_like(img)
        hip.aug_crop_multi(desc, 2, table, pk, ref, lab, ROI)
        hip.aug_crop_affine(desc, 2, table, pk, eye, img, lab, ROI, -0.6974)
        assert torch.equal(img, ref), "identity matrices must reproduce the plain gather"
        t = alternate([lambda: hip.aug_crop_multi(desc, 2, table, pk, img, lab, ROI),
                       lambda: hip.aug_crop_affine(desc, 2, table, pk, eye, img, lab, ROI, -0.6974),
                       lambda: hip.aug_crop_affine(desc, 2, table, pk, rnd, img, lab, ROI, -0.6974)])
        print(f"{chans:3d}  {str(dtype).split('.')[-1]:>8s} | {t[0]:9.2f}   {t[1]:9.2f} ({t[1] / t[0]:5.2f} x, {100 * t[1] / STEP_US:5.2f} %)"
              f"              {t[2]:9.2f} ({t[2] / t[0]:5.2f} x, {100 * t[2] / STEP_US:5.2f} %)", flush=True)
