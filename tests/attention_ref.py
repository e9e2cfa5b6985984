"""Plain-torch CPU float64 restatement of the shifted-window attention core between the qkv Linear and the proj Linear, written
from the algorithm (Liu et al. 2021, 3-D as in nnFormer / MONAI's SwinUNETR) on the window helpers of ``oracle.swin``; used by
the tests only, no project kernel involved.  ``tests/test_attention_ref_host.py`` pins it to ``oracle.swin.WindowAttention`` /
``SwinTransformerBlock`` and to the committed ``tests/golden/swin_attn_*.npz`` before ``tests/test_gpu_attention_ref.py`` trusts
it at other shapes.

What it computes, in order: pad every axis to a window multiple (a padded token's qkv is ``qkv_bias``: the reference pads
BEFORE its qkv Linear, and Linear(0) = bias); roll by -shift; partition into windows; q.k * hd^-1/2 + table[index] + mask (the
-100 region mask on the PADDED grid, only when shift > 0); softmax; P.V; reverse the windows; roll back; crop.

``VARIANTS`` names deliberately wrong versions of it (``_variant=``): the method check of the host test shows that the GPU tests
would catch each of them.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.swin import relative_position_index, shift_region_mask, window_partition, window_reverse

VARIANTS = ("mask_unpadded",      # region mask built on the unpadded grid
            "swap_hw",            # H and W swapped in the partition
            "pad_zero",           # padded tokens are zeros instead of the bias
            "subcube_index",      # bias_ws > ws: the [:ws, :ws, :ws] sub-cube of the bias_ws grid instead of MONAI's linear slice
            "index_transposed")   # bias index transposed (key - query instead of query - key)


def _pad_to(L, ws):
    return -(-L // ws) * ws


def bias_index(ws, bias_ws=None, _variant=None):
    """[ws^3, ws^3] index into the (2 bias_ws - 1)^3 table.  bias_ws > ws is MONAI's slice of the bias_ws index: token i takes
    position i of the bias_ws grid in LINEAR order, not the ws^3 sub-cube."""
    bws = bias_ws or ws
    N = ws ** 3
    full = relative_position_index(bws)
    if _variant == "subcube_index" and bws > ws:
        r = torch.arange(ws)
        pos = (r[:, None, None] * bws * bws + r[None, :, None] * bws + r[None, None, :]).reshape(-1)
        idx = full[pos][:, pos]
    else:
        idx = full[:N, :N]
    return idx.t() if _variant == "index_transposed" else idx


def window_attention_ref(qkv, qkv_bias, table, heads, ws, shift, bias_ws=None, _variant=None):
    """qkv [B,S,H,W,3C] (channel = which*C + head*hd + e), qkv_bias [3C] or None, table [M3, heads] or per sample [B, M3, heads]
    -> (out [B,S,H,W,C], lse [B*nW, heads, ws^3] in the kernel's layout, pmax [B,S,H,W,heads]: the largest probability of every
    query row).  Everything float64; gradients come from autograd on this graph."""
    assert _variant is None or _variant in VARIANTS
    assert qkv.dtype == torch.float64 and table.dtype == torch.float64 and not qkv.is_cuda
    B, S, H, W, C3 = qkv.shape
    C, N = C3 // 3, ws ** 3
    hd = C // heads
    Sp, Hp, Wp = _pad_to(S, ws), _pad_to(H, ws), _pad_to(W, ws)
    x = F.pad(qkv, (0, 0, 0, Wp - W, 0, Hp - H, 0, Sp - S))
    if qkv_bias is not None and _variant != "pad_zero":
        real = torch.zeros(Sp, Hp, Wp, 1, dtype=torch.bool)
        real[:S, :H, :W] = True
        x = torch.where(real, x, qkv_bias.to(torch.float64))
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift, -shift), dims=(1, 2, 3))
    swap = _variant == "swap_hw"
    if swap:
        x = x.transpose(2, 3)
    win = window_partition(x, ws)                                             # [B*nW, ws, ws, ws, 3C]
    nW = win.shape[0] // B
    q, k, v = win.reshape(B * nW, N, 3, heads, hd).permute(2, 0, 3, 1, 4)     # each [B*nW, heads, N, hd]
    attn = (q @ k.transpose(-2, -1)) * hd ** -0.5
    idx = bias_index(ws, bias_ws, _variant)
    if table.dim() == 2:
        bias = table[idx].permute(2, 0, 1)[None]                              # [1, heads, N, N]
    else:
        bias = table[:, idx].permute(0, 3, 1, 2).repeat_interleave(nW, dim=0)  # window b * nW + w takes the table of sample b
    attn = attn + bias
    if shift > 0:
        if _variant == "mask_unpadded":
            ids = []
            for L, Lp in ((S, Sp), (H, Hp), (W, Wp)):
                r = torch.zeros(Lp, dtype=torch.long)
                r[max(L - ws, 0):L - shift] = 1
                r[L - shift:] = 2
                ids.append(r)
            vol = (ids[0][:, None, None] * 9 + ids[1][None, :, None] * 3 + ids[2][None, None, :]).double()
            w_ = window_partition(vol[None, ..., None], ws).reshape(-1, N)
            mask = torch.where(w_[:, None, :] != w_[:, :, None], -100.0, 0.0).double()
        else:
            mask = shift_region_mask(*((Sp, Wp, Hp) if swap else (Sp, Hp, Wp)), ws, shift).double()
        attn = (attn.reshape(B, nW, heads, N, N) + mask[None, :, None]).reshape(B * nW, heads, N, N)
    lse = torch.logsumexp(attn, dim=-1)
    prob = torch.softmax(attn, dim=-1)
    out = (prob @ v).transpose(1, 2).reshape(B * nW, ws, ws, ws, C)
    pmax = prob.max(dim=-1).values.transpose(1, 2).reshape(B * nW, ws, ws, ws, heads)

    def back(t):
        if swap:
            t = window_reverse(t, ws, Sp, Wp, Hp).transpose(2, 3)
        else:
            t = window_reverse(t, ws, Sp, Hp, Wp)
        if shift > 0:
            t = torch.roll(t, shifts=(shift, shift, shift), dims=(1, 2, 3))
        return t[:, :S, :H, :W, :]

    return back(out), lse, back(pmax.detach())
