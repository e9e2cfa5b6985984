"""Forward + backward time of the three loss kinds (DiceCE, Tversky, DiceFocal), and of their sigmoid forms under a region
table (--label_regions; `regions:` rows), on what the UNet hands over at the flagship shape: channels-last bf16 logits rows 2 x 96^3 x 8 (3 classes valid), fp32 labels, gradient rows written in the same layout.
A pair is the three launches a criterion issues (partials, rows finalize, backward).  All kinds move the same bytes (35.4 MB
forward, 63.7 MB backward), so DiceCE's time from the same run is the yardstick.  The kinds are timed in alternation: ROUNDS
replays each of a captured graph of REPS pairs, between device events; median / min / max of the per-pair times in us.
The passes are called directly (hip.seg_loss_fwd / seg_loss_bwd): every operation of the capture is issued inside it, with no
autograd node from outside the capture to run on another stream.
usage: python tools/bench_losses.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from medicalsemseg_amd import hip

ROUNDS, REPS = 7, 20
dev = torch.device("cuda:0")
N, C, LD, vol = 2, 3, 8, (96, 96, 96)
torch.manual_seed(0)
rows = (torch.randn(N, *vol, LD, device=dev) * 2).to(torch.bfloat16)
logits = rows[..., :C].permute(0, 4, 1, 2, 3)
labels = torch.randint(0, C, (N, 1) + vol, device=dev).float()
drows = torch.empty_like(rows)
gscale = torch.ones(1, device=dev)
REGIONS = (0b110, 0b100, 0b010)      # three overlapping regions over the label values 0..2
kinds = {"DiceCE": (hip.LOSS_DICE_CE, 0.0, 0.0), "Tversky": (hip.LOSS_TVERSKY, 0.3, 0.7), "DiceFocal": (hip.LOSS_DICE_FOCAL, 0.0, 0.0)}
kinds.update({"regions:" + k: v + (REGIONS,) for k, v in list(kinds.items())})


def pair(kind, alpha, beta, regions=None):
    partial, _, loss3 = hip.seg_loss_fwd(logits, labels, C, 1e-5, 1e-5, kind, alpha, beta, LD, want_hard=True, regions=regions)
    hip.seg_loss_bwd(logits, labels, partial, gscale, drows, C, 1e-5, 1e-5, kind, alpha, beta, LD, LD, regions=regions)
    return loss3


# REPS pairs per kind in one captured graph: issued from Python a pair costs more host time than its ~20 us of kernels
graphs, losses = {}, {}
for name, args in kinds.items():
    for _ in range(3):
        pair(*args)
    torch.cuda.synchronize()
    graphs[name] = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graphs[name]):
        for _ in range(REPS):
            losses[name] = pair(*args)
    graphs[name].replay()
torch.cuda.synchronize()
times = {k: [] for k in kinds}
for _ in range(ROUNDS):
    for name, g in graphs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / REPS)
base = sorted(times["DiceCE"])[ROUNDS // 2]
for name, ts in times.items():
    ts.sort()
    print(f"{name:17s} fwd + bwd, {N} x {C} x 96^3 bf16 rows of {LD}: median {ts[ROUNDS // 2]:.1f} us, min {ts[0]:.1f}, "
          f"max {ts[-1]:.1f} over {ROUNDS} replays of {REPS} pairs; {ts[ROUNDS // 2] / base:.2f} x DiceCE; "
          f"loss {float(losses[name][0]):.5f}")
