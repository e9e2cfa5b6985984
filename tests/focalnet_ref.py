"""Plain-torch CPU restatement of the FocalNet encoder, written from the algorithm (focal modulation: Yang et al. 2022, as the
3-D encoder the reference wires into SwinUNETRCustom); used by the tests only.  It is pinned to
``tests/golden/focalnet_encoder_v32.npz`` (what the reference's own class computes, ``tools/gen_golden_focalnet.py``) in
``tests/test_focalnet_host.py`` and then serves as the checker at other shapes and dtypes.

Module and parameter names equal the reference's state-dict keys, so weights move by ``load_state_dict``.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


class PatchEmbedRef(nn.Module):
    def __init__(self, k, cin, cout):
        super().__init__()
        self.proj = nn.Conv3d(cin, cout, kernel_size=k, stride=k)
        self.norm = nn.LayerNorm(cout)

    def forward(self, x):                       # [B, C, D, H, W] -> [B, C', D/k, H/k, W/k]
        x = self.proj(x)
        return self.norm(x.permute(0, 2, 3, 4, 1)).permute(0, 4, 1, 2, 3)


class MlpRef(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class FocalModulationRef(nn.Module):
    def __init__(self, dim, focal_window, focal_level=2):
        super().__init__()
        self.dim, self.focal_level = dim, focal_level
        self.f = nn.Linear(dim, 2 * dim + focal_level + 1)
        self.h = nn.Conv3d(dim, dim, kernel_size=1)
        self.proj = nn.Linear(dim, dim)
        self.focal_layers = nn.ModuleList()
        for l in range(focal_level):
            k = 2 * l + focal_window
            self.focal_layers.append(nn.Sequential(nn.Conv3d(dim, dim, kernel_size=k, padding=k // 2, groups=dim, bias=False)))

    def forward(self, x):                       # [B, D, H, W, C]
        C, L = self.dim, self.focal_level
        y = self.f(x).permute(0, 4, 1, 2, 3)
        q, ctx, gates = y[:, :C], y[:, C:2 * C], y[:, 2 * C:]
        ctx_all = 0
        for l in range(L):
            ctx = F.gelu(self.focal_layers[l][0](ctx))
            ctx_all = ctx_all + ctx * gates[:, l:l + 1]
        ctx_all = ctx_all + F.gelu(ctx.mean((2, 3, 4), keepdim=True)) * gates[:, L:L + 1]
        out = q * self.h(ctx_all)
        return self.proj(out.permute(0, 2, 3, 4, 1))


class FocalBlockRef(nn.Module):
    def __init__(self, dim, focal_window, mlp_ratio):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.modulation = FocalModulationRef(dim, focal_window)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MlpRef(dim, int(dim * mlp_ratio))

    def forward(self, x):                       # stochastic depth is off in every use of this checker
        x = x + self.modulation(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class FocalLayerRef(nn.Module):
    def __init__(self, dim, depth, focal_window, mlp_ratio):
        super().__init__()
        self.blocks = nn.ModuleList([FocalBlockRef(dim, focal_window, mlp_ratio) for _ in range(depth)])
        self.downsample = PatchEmbedRef(2, dim, 2 * dim)

    def forward(self, x):                       # [B, D, H, W, C] -> [B, D/2, H/2, W/2, 2C]
        for b in self.blocks:
            x = b(x)
        return self.downsample(x.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)


class FocalNetRef(nn.Module):
    """signature and outputs of oracle.swin.SwinTransformerNNFormer, so oracle.swin.SwinUNETRCustom takes it: a list of
    NCDHW feature maps [C@R, 2C@R/2, ...]"""

    def __init__(self, pretrain_img_size=(96, 96, 96), patch_size=(2, 2, 2), in_chans=1, embed_dim=48, depths=(2, 2, 2, 2),
                 focal_windows=(9, 9, 9, 9), mlp_ratio=4.0):
        super().__init__()
        self.num_layers = len(depths)
        self.patch_embed = PatchEmbedRef(tuple(patch_size), in_chans, embed_dim)
        self.layers = nn.ModuleList([FocalLayerRef(embed_dim * 2 ** i, depths[i], focal_windows[i], mlp_ratio)
                                     for i in range(self.num_layers)])
        for i in range(self.num_layers):
            self.add_module(f"norm{i}", nn.LayerNorm(embed_dim * 2 ** (i + 1)))

    def forward(self, inp):
        vol = inp[0] if isinstance(inp, (tuple, list)) else inp
        x = self.patch_embed(vol)
        outs = [x]
        x = x.permute(0, 2, 3, 4, 1)
        for i, layer in enumerate(self.layers):
            x = layer(x)
            outs.append(getattr(self, f"norm{i}")(x).permute(0, 4, 1, 2, 3).contiguous())
        return outs
