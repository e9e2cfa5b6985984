"""Whole-step time of FocalNetUNETR-48 (depths 2-2-2-2, focal windows 9: depthwise kernels 9^3 / 11^3) at 96^3, batch 2, bf16:
forward + DiceCE + backward + FlatAdamW, replayed from a captured hipGraph; warm-up, then replays timed with device events
until at least a second has passed; median / min / max in ms.
usage: python tools/bench_focalnet_step.py [focal_window]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from medicalsemseg_amd import layers
from medicalsemseg_amd.losses import DiceCELoss
from medicalsemseg_amd.models import swin_unetr as P
from medicalsemseg_amd.models.focalnet import FocalNet
from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay

fw = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
vol, hs, B = (96, 96, 96), 48, 2
torch.manual_seed(0)
enc = FocalNet(vol, patch_size=(2, 2, 2), in_chans=1, embed_dim=hs, depths=(2, 2, 2, 2), focal_windows=(fw,) * 4,
               compute_dtype=torch.bfloat16, drop_path_rate=0.0)
net = P.SwinUNETRCustom(enc, 1, 3, vol, hs, (2, 2, 2), compute_dtype=torch.bfloat16).to(dev)
opt = FlatAdamW(add_weight_decay(net, 1e-5), lr=4e-4, betas=(0.9, 0.95), eps=1e-6)
crit = DiceCELoss()
x = torch.randn(B, 1, *vol, device=dev)
y = torch.randint(0, 3, (B, 1) + vol, device=dev).float()


def step():
    loss = crit(net((x, None, None)), y)
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss


for _ in range(2):
    step()
torch.cuda.synchronize()
layers.PACK_REGISTRY.prepare()
layers.bump_weights_epoch()
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    sl = step()
for _ in range(3):
    g.replay()
torch.cuda.synchronize()
ts = []
while sum(ts) < 1000.0 or len(ts) < 10:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
ts.sort()
print(f"FocalNetUNETR-48 window {fw} 96^3 B={B} bf16 step (graph replay): median {ts[len(ts) // 2]:.3f} ms, min {ts[0]:.3f}, "
      f"max {ts[-1]:.3f} over {len(ts)} replays; loss {float(sl):.4f}")
