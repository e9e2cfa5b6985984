"""Step time of Swin-UNETR-48 (nnFormerUNETR, the config of ``bench.py --workload swin_unetr``: 96^3, batch 2, bf16) with the
spacing-conditioned relative position bias (``--rel_pos_bias_affine``) off and on.

One model is built with the flag on.  The flag-off step feeds it ``affine = None``, which runs exactly the flag-off
model's launches (tests/test_gpu_affine_bias.py checks that bit for bit); the flag-on step feeds a static device tensor of
per-sample spacings.  Each step (forward + DiceCE loss + backward + AdamW + zero_grad) is captured in its own hipGraph, as
bench.py does (``--no-graph``: eager launches), and the two are replayed alternately, ``--steps`` replays per leg and
``--rounds`` rounds after warm-up.  The kernels' own times come from a separate run under
``rocprofv3 --kernel-trace --stats``.

    python tools/bench_affine_bias.py [--steps 20] [--rounds 5] [--no-graph]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()

    from bench import synth_batch
    from medicalsemseg_amd import layers
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models.swin_unetr import SwinTransformerNNFormer, SwinUNETRCustom
    from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay

    dev = torch.device("cuda:0")
    torch.manual_seed(13)
    dtype = torch.bfloat16
    enc = SwinTransformerNNFormer((args.size,) * 3, (2, 2, 2), 1, 48, (2, 2, 2, 2), (3, 6, 12, 24), (6, 6, 6, 3),
                                  drop_path_rate=0.0, compute_dtype=dtype, rel_pos_bias_affine=True)
    net = SwinUNETRCustom(enc, 1, 3, (args.size,) * 3, 48, (2, 2, 2), compute_dtype=dtype).to(dev)
    opt = FlatAdamW(add_weight_decay(net, 1e-5), lr=4e-4, betas=(0.9, 0.95), eps=1e-6)
    crit = DiceCELoss(smooth_nr=1e-5, smooth_dr=1e-5)
    x, y = synth_batch(args.batch, args.size, 3, dev, 13)
    aff = torch.tensor([[1.5, 0.8, 2.0], [-0.7, 1.25, 3.0]] * (args.batch // 2 + 1), device=dev)[:args.batch].contiguous()

    def step(a):
        loss = crit(net((x, None, a)), y)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    legs = {"off": lambda: step(None), "on": lambda: step(aff)}
    for _ in range(max(args.warmup, 1)):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    graphs = {}
    if not args.no_graph:
        for name, f in legs.items():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                f()
            torch.cuda.current_stream().wait_stream(side)
            layers.PACK_REGISTRY.prepare()
            layers.bump_weights_epoch()          # the capture includes the weight re-packing, as in bench.py
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                f()
            graphs[name] = g
            g.replay()
            torch.cuda.synchronize()

    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                if graphs:
                    graphs[name].replay()
                else:
                    f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"workload": "swin_unetr rel_pos_bias_affine", "graph": bool(graphs), "steps": args.steps,
                      "rounds": args.rounds, "ms_per_step_off": round(med["off"], 4), "ms_per_step_on": round(med["on"], 4),
                      "on_over_off": round(med["on"] / med["off"], 4),
                      "rounds_ms": {k: [round(t, 4) for t in v] for k, v in times.items()}}))


if __name__ == "__main__":
    main()
