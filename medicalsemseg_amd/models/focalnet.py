"""FocalNet encoder on the HIP kernels: mirror of ``/root/reference/models/backbones/focalnet_3d.py`` (``FocalNet``
:318-471, ``BasicLayer`` :178-258, ``FocalModulationBlock`` :109-175, ``FocalModulation`` :39-106) with the options the
reference's builder leaves off (``use_postln``, ``use_layerscale``, ``use_conv_embed``) not implemented.  It returns the
same five channels-last feature maps as ``SwinTransformerNNFormer``, so ``SwinUNETRCustom`` takes it unchanged
(``models/model_builder.py:225-241`` of the reference).  Parameter names and order equal the reference's.

A focal modulation block replaces window attention by two depthwise convolutions (kernel ``focal_window`` and
``focal_window + 2``: 9^3 and 11^3 at the defaults) of a context tensor, gated per voxel and modulating a query:
``ops.FocalModulationFn`` over ``csrc/depthwise_large.hip`` and ``csrc/focal.hip``.  Tokens are channels-last volumes, so
the reference's permute / contiguous pairs around the convolutions do not exist; ``q | ctx | gates`` stay views of the one
``f`` output.  ``f`` has 2C + 3 outputs: it runs zero-padded to 2C + 8 (``_PaddedState``), the state dict shows the
reference's shapes.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from .. import hip, ops
from .swin_unetr import _Mlp, _PaddedState, _PatchEmbed3D, _p8

FOCAL_LEVEL = 2          # the reference's focal_levels default; its builder passes nothing else
MIN_WINDOW, MAX_WINDOW = 3, 9    # focal_window + 2 * (FOCAL_LEVEL - 1) <= 11, the largest depthwise kernel


class _FocalF(nn.Linear, _PaddedState):
    """Linear(dim, 2 dim + 3) -> q | ctx | gates, the output rows zero-padded to a multiple of 8"""

    def __init__(self, dim):
        real = 2 * dim + FOCAL_LEVEL + 1
        nn.Linear.__init__(self, dim, _p8(real))     # the default initialisation depends on the fan-in only
        self._real = {"weight": (real, dim), "bias": (real,)}
        self._init_padded()


class _FocalConv(nn.Sequential):
    """`nn.Sequential(Conv3d(groups=dim, bias=False), GELU())` of the reference: only the state-dict name `0.weight`"""

    def __init__(self, dim, k):
        super().__init__(nn.Conv3d(dim, dim, kernel_size=k, stride=1, groups=dim, padding=k // 2, bias=False))


class _FocalModulation(nn.Module):
    def __init__(self, dim, focal_window):
        super().__init__()
        self.dim = dim
        self.f = _FocalF(dim)
        self.h = nn.Conv3d(dim, dim, kernel_size=1, stride=1, padding=0, groups=1, bias=True)
        self.proj = nn.Linear(dim, dim)
        self.focal_layers = nn.ModuleList([_FocalConv(dim, 2 * k + focal_window) for k in range(FOCAL_LEVEL)])

    def core(self, xn):
        """everything before `proj`"""
        f = ops.linear(xn, self.f.weight, self.f.bias)
        return ops.focal_modulation(f, self.focal_layers[0][0].weight, self.focal_layers[1][0].weight, self.h.weight, self.h.bias)


class _FocalBlock(nn.Module):
    def __init__(self, dim, focal_window, mlp_ratio, drop_path):
        super().__init__()
        self.drop_path = float(drop_path)
        self.norm1 = nn.LayerNorm(dim)
        self.modulation = _FocalModulation(dim, focal_window)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))

    def _dp_scale(self, x):
        """per-sample stochastic-depth factor mask[b] / keep, or None (as swin_unetr._Block); `self.dp_mask` overrides the draw"""
        if self.drop_path == 0.0 or not self.training:
            return None
        keep = 1.0 - self.drop_path
        mask = getattr(self, "dp_mask", None)
        if mask is None:
            mask = torch.empty(x.shape[0], device=x.device, dtype=torch.float32).bernoulli_(keep)
        return mask.to(device=x.device, dtype=torch.float32) / keep

    def forward(self, x):
        mod, mlp = self.modulation, self.mlp
        x, xn = ops.layer_norm_res(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        y = mod.core(xn)
        dp = self._dp_scale(x)
        if dp is None:
            x = ops.linear_add(y, mod.proj.weight, mod.proj.bias, x)
        else:
            x = ops.add(x, ops.linear(y, mod.proj.weight, mod.proj.bias), dp)
        x, y = ops.layer_norm_res(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        dp = self._dp_scale(x)
        if dp is None:
            return ops.mlp(y, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, res=x)
        return ops.add(x, ops.mlp(y, mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias), dp)


class _FocalLayer(nn.Module):
    def __init__(self, dim, depth, focal_window, mlp_ratio, drop_path):
        super().__init__()
        self.blocks = nn.ModuleList([_FocalBlock(dim, focal_window, mlp_ratio, drop_path[i]) for i in range(depth)])
        self.downsample = _PatchEmbed3D((2, 2, 2), dim, 2 * dim)     # every stage, the last included (:393)

    def forward(self, x):
        for b in self.blocks:
            x = b(x)
        return self.downsample(x)


class FocalNet(nn.Module):
    """returns the 5 feature volumes channels-last: [C@R, 2C@R/2, 4C@R/4, 8C@R/8, 16C@R/16] (R = vol / patch) and the
    channels-last input, like SwinTransformerNNFormer."""

    def __init__(self, pretrain_img_size=(96, 96, 96), patch_size=(2, 2, 2), in_chans=1, embed_dim=48,
                 depths: Sequence[int] = (2, 2, 2, 2), focal_windows: Sequence[int] = (9, 9, 9, 9), mlp_ratio=4.0,
                 drop_path_rate=0.2, compute_dtype=torch.bfloat16):
        super().__init__()
        if len(focal_windows) != len(depths):
            raise NotImplementedError(f"focal_windows {tuple(focal_windows)} must give one window per stage ({len(depths)})")
        for w in focal_windows:
            if w % 2 == 0 or not MIN_WINDOW <= w <= MAX_WINDOW:
                raise NotImplementedError(f"focal window {w}: odd windows {MIN_WINDOW}..{MAX_WINDOW} are implemented (depthwise "
                                          f"kernels 3..11; an even window fails in the reference itself)")
        if embed_dim % 8:
            raise NotImplementedError(f"embed_dim {embed_dim}: the depthwise kernels take channel counts that are a multiple of 8")
        self.num_layers, self.embed_dim, self.compute_dtype = len(depths), embed_dim, compute_dtype
        self.patch_embed = _PatchEmbed3D(patch_size, in_chans, embed_dim)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList([_FocalLayer(embed_dim * 2 ** i, depths[i], focal_windows[i], mlp_ratio,
                                                 dpr[sum(depths[:i]):sum(depths[:i + 1])]) for i in range(self.num_layers)])
        self.num_features = [embed_dim * 2 ** (i + 1) for i in range(self.num_layers)]
        for i in range(self.num_layers):
            self.add_module(f"norm{i}", nn.LayerNorm(self.num_features[i]))

    def forward(self, inp):
        vol = inp[0] if isinstance(inp, (tuple, list)) else inp
        if not vol.is_cuda:
            raise RuntimeError("FocalNet runs on the GPU only (no CPU fallback)")
        B, Cin, D, H, W = vol.shape
        p = self.patch_embed.patch_size[0]
        if D % (p << self.num_layers) or H % (p << self.num_layers) or W % (p << self.num_layers):
            raise ValueError(f"volume must be a multiple of patch_size * 2^num_layers = {p << self.num_layers}")
        x_cl = torch.empty(B, D, H, W, Cin, dtype=self.compute_dtype, device=vol.device)
        hip.to_channels_last(vol if vol.dtype in (torch.float32, torch.bfloat16) else vol.float(), x_cl)
        x = self.patch_embed(x_cl)
        feats = [x]
        for i, layer in enumerate(self.layers):
            x = layer(x)
            n = getattr(self, f"norm{i}")
            feats.append(ops.layer_norm(x, n.weight, n.bias, n.eps))   # norm of the DOWNSAMPLED tensor (:463-469)
        return feats, x_cl
