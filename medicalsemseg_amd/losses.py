"""Dice + cross-entropy, Tversky and Dice + focal losses and the hard Dice metric on the fused HIP reductions.

``DiceCELoss`` keeps the call signature of ``monai.losses.DiceCELoss`` as the reference constructs it
(``/root/reference/run_training.py:103-105``: ``to_onehot_y=True, softmax=True, squared_pred=True,
smooth_nr, smooth_dr``) and calls it (``/root/reference/engine/train.py:62``: ``criterion(logits[B,C,...],
labels[B,1,...]) -> 0-dim tensor``).  One pass over logits+labels produces every reduction of the loss AND of
the per-step hard Dice metric (``engine/train.py:89-111``); the backward is a second single pass.

``TverskyLoss`` and ``DiceFocalLoss`` are the other two criteria of the reference's ``--loss_fn`` switch
(its ``run_training.py:106-115``), with MONAI's definitions, on the same two passes (a loss kind selects what the
kernels accumulate).  The focal term of ``DiceFocalLoss`` is MONAI's SIGMOID focal loss (gamma 2) on the raw logits:
``monai.losses.DiceFocalLoss`` hands its ``softmax`` flag to the Dice half only.
"""
from __future__ import annotations

import torch

from . import hip


import weakref

# gradients this module wrote as channels-last rows [N, *spatial, ld] with ZERO padding channels, keyed by data_ptr:
# a model whose logits are a [B, C, ...] view of such rows (models/unet.py) takes them back without a layout pass
_CL_GRADS = weakref.WeakValueDictionary()


def _channels_last_rows(t: torch.Tensor):
    """ld if `t` [N, C, *spatial] is the channel-first VIEW of dense channels-last rows [N, *spatial, ld] (ld >= C,
    unit channel stride), else 0."""
    if t.dim() < 3 or t.stride(1) != 1 or t.shape[1] == 1:
        return 0
    ld = t.stride(-1)
    exp = ld
    for d in range(t.dim() - 1, 1, -1):
        if t.stride(d) != exp:
            return 0
        exp *= t.shape[d]
    if t.stride(0) != exp or ld < t.shape[1]:
        return 0
    return ld


def channels_last_grad(g: torch.Tensor, ld: int, dtype):
    """[N, *spatial, ld] tensor behind `g` if `g` is a gradient produced by _SegLossFn.backward in that layout, else None"""
    base = _CL_GRADS.get(g.data_ptr())
    if base is None or base.dtype != dtype or base.shape[-1] != ld or _channels_last_rows(g) != ld:
        return None
    if base.shape[0] != g.shape[0] or tuple(base.shape[1:-1]) != tuple(g.shape[2:]) or base.device != g.device:
        return None
    return base


class _SegLossFn(torch.autograd.Function):
    """one fused forward pass and one fused backward pass for every loss kind (hip.LOSS_*)"""

    @staticmethod
    def forward(ctx, logits, labels, smooth_nr, smooth_dr, kind, alpha, beta, holder, name, regions=None):
        if not logits.is_cuda:
            raise RuntimeError(f"{name} runs on the GPU only (no CPU fallback)")
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.float()
        ld = _channels_last_rows(logits)
        if ld == 0 or logits.data_ptr() % 16 or (ld * logits.element_size()) % 16:
            ld = 0
            logits = logits.contiguous()
        labels = labels.contiguous()
        if labels.dtype not in (torch.float32, torch.bfloat16, torch.uint8, torch.int64):
            labels = labels.long()
        N, C = logits.shape[0], logits.shape[1]
        S = logits.numel() // (N * C)
        if labels.numel() != N * S:
            raise ValueError(f"labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
        if N <= 8:   # deterministic two-step reduction (no atomics, no zero-filled outputs)
            partial, hard, loss3 = hip.seg_loss_fwd(logits, labels, C, smooth_nr, smooth_dr, kind, alpha, beta, ld,
                                                    want_hard=True, regions=regions)
        else:
            partial, hard = hip.seg_loss_partials(logits, labels, C, kind, ld, want_hard=True, regions=regions)
            loss3 = hip.seg_loss_finalize(partial, S, smooth_nr, smooth_dr, kind, alpha, beta, regions=regions)
        ctx.save_for_backward(logits, labels, partial)
        ctx.cfg = (smooth_nr, smooth_dr, kind, alpha, beta)
        ctx.regions = regions
        ctx.ld = ld
        if holder is not None:
            holder["hard"] = hard          # [N, C, 3] = (|P&T|, |P|, |T|) for the metric
            holder["parts"] = loss3        # (total, dice, ce) | (total, tversky, 0) | (total, dice, focal)
            holder["of"] = (logits.data_ptr(), tuple(logits.shape))   # which logits these by-products belong to
        return loss3[0]

    @staticmethod
    def backward(ctx, g):
        logits, labels, partial = ctx.saved_tensors
        N, C = logits.shape[0], logits.shape[1]
        gs = g.reshape(1).to(torch.float32).contiguous()
        none = (None,) * 9
        if ctx.ld:
            # logits are a view of channels-last rows: the gradient goes out in the same layout (padding channels zeroed
            # by the kernel) and is registered so that the producer of the logits can take the rows as they are
            rows = torch.empty((N,) + tuple(logits.shape[2:]) + (ctx.ld,), dtype=logits.dtype, device=logits.device)
            hip.seg_loss_bwd(logits, labels, partial, gs, rows, C, *ctx.cfg, ctx.ld, ctx.ld, regions=ctx.regions)
            _CL_GRADS[rows.data_ptr()] = rows
            perm = (0, logits.dim() - 1) + tuple(range(1, logits.dim() - 1))
            return (rows[..., :C].permute(*perm),) + none
        dl = torch.empty_like(logits)
        hip.seg_loss_bwd(logits, labels, partial, gs, dl, C, *ctx.cfg, 0, 0, regions=ctx.regions)
        return (dl,) + none


class _FusedLoss(torch.nn.Module):
    """what the three criteria share: the smoothing terms, the by-products of the last call and the call itself"""
    kind = hip.LOSS_DICE_CE
    alpha = beta = 0.0

    def __init__(self, smooth_nr, smooth_dr, regions=None):
        super().__init__()
        self.smooth_nr, self.smooth_dr = float(smooth_nr), float(smooth_dr)
        self.last = {}   # by-products of the last call: 'hard' counts and the loss triple 'parts'
        # region-based training: a tuple of uint32 bit masks, one per logits channel (bit l set: label value l belongs to the
        # region), or the (masks, values) pair of arguments.parse_label_regions.  The criterion is then the SIGMOID form of
        # its kind: every channel on its own against t = (mask[c] >> label) & 1, the cross-entropy term a BCE-with-logits
        # mean over N*C*S; 'hard' holds (|P_c & T_c|, |P_c|, |T_c|) per region with P_c = (logit > 0)
        if regions is not None and len(regions) == 2 and isinstance(regions[0], (tuple, list)):
            regions = regions[0]
        self.regions = None if regions is None else tuple(int(m) for m in regions)

    def forward(self, logits, labels):
        if logits.shape[1] > 16:
            raise ValueError("at most 16 classes are supported")
        if self.regions is not None and len(self.regions) != logits.shape[1]:
            raise ValueError(f"{len(self.regions)} regions for logits of {logits.shape[1]} channels")
        return _SegLossFn.apply(logits, labels, self.smooth_nr, self.smooth_dr, self.kind, self.alpha, self.beta, self.last,
                                type(self).__name__, self.regions)


class DiceCELoss(_FusedLoss):
    def __init__(self, to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=1e-5, smooth_dr=1e-5,
                 include_background=True, lambda_dice=1.0, lambda_ce=1.0, regions=None):
        if not (to_onehot_y and softmax and squared_pred and include_background) or lambda_dice != 1.0 or lambda_ce != 1.0:
            raise ValueError("only the reference's configuration is implemented: to_onehot_y=True, softmax=True, "
                             "squared_pred=True, include_background=True, lambda_dice=lambda_ce=1")
        super().__init__(smooth_nr, smooth_dr, regions)


class TverskyLoss(_FusedLoss):
    """``monai.losses.TverskyLoss(to_onehot_y=True, softmax=True, alpha, beta, smooth_nr, smooth_dr)``: per (n, c)
    ``1 - (I + smooth_nr) / (I + alpha * FP + beta * FN + smooth_dr)`` with ``FP = sum p - I``, ``FN = sum t - I`` (no squared
    prediction), averaged over (n, c).  ``last['parts']`` is (loss, loss, 0)."""
    kind = hip.LOSS_TVERSKY

    def __init__(self, to_onehot_y=True, softmax=True, alpha=0.5, beta=0.5, smooth_nr=1e-5, smooth_dr=1e-5,
                 include_background=True, regions=None):
        if not (to_onehot_y and softmax and include_background):
            raise ValueError("only the reference's configuration is implemented: to_onehot_y=True, softmax=True, "
                             "include_background=True")
        super().__init__(smooth_nr, smooth_dr, regions)
        self.alpha, self.beta = float(alpha), float(beta)


class DiceFocalLoss(_FusedLoss):
    """``monai.losses.DiceFocalLoss(to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr, smooth_dr)``: DiceCELoss's
    Dice term plus MONAI's focal term, which is the SIGMOID focal loss (gamma 2) of the raw logits against the one-hot labels,
    averaged over all N*C*S elements -- DiceFocalLoss does not hand ``softmax`` to its FocalLoss.  ``last['parts']`` is
    (loss, dice, focal)."""
    kind = hip.LOSS_DICE_FOCAL

    def __init__(self, to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr=1e-5, smooth_dr=1e-5,
                 include_background=True, gamma=2.0, lambda_dice=1.0, lambda_focal=1.0, regions=None):
        if (not (to_onehot_y and softmax and squared_pred and include_background) or gamma != 2.0 or lambda_dice != 1.0
                or lambda_focal != 1.0):
            raise ValueError("only the reference's configuration is implemented: to_onehot_y=True, softmax=True, "
                             "squared_pred=True, include_background=True, gamma=2, lambda_dice=lambda_focal=1")
        super().__init__(smooth_nr, smooth_dr, regions)


def build_criterion(cfg):
    """the criterion ``--loss_fn`` names (DiceCE | Tversky | DiceFocal), in the reference's configuration
    (its ``run_training.py:103-115``); under ``--label_regions`` its sigmoid form on the flag's region table"""
    from .utils.arguments import region_table
    table = region_table(cfg)
    smooth = dict(smooth_nr=cfg.smooth_nr, smooth_dr=cfg.smooth_dr, regions=None if table is None else table[0])
    makers = {"DiceCE": lambda: DiceCELoss(**smooth),
              "Tversky": lambda: TverskyLoss(alpha=cfg.tversky_alpha, beta=cfg.tversky_beta, **smooth),
              "DiceFocal": lambda: DiceFocalLoss(**smooth)}
    if cfg.loss_fn not in makers:
        raise RuntimeError("Could not parse loss function argument.")
    return makers[cfg.loss_fn]()


def dice_from_counts(hard: torch.Tensor):
    """hard [N,C,3] -> (scores[N,C] with NaN where |T| == 0, not_nans[N,C]) like MONAI
    ``DiceMetric(include_background=True, reduction='none', get_not_nans=True).aggregate()``."""
    inter, p, t = hard[..., 0], hard[..., 1], hard[..., 2]
    score = torch.where(t > 0, 2.0 * inter / (p + t), torch.full_like(inter, float("nan")))
    return score, (~torch.isnan(score)).float()


def dice_metric(logits: torch.Tensor, labels: torch.Tensor, regions=None):
    """argmax one-hot hard Dice per (n, c) in one fused pass (replaces decollate + AsDiscrete + DiceMetric,
    ``/root/reference/engine/train.py:89-94``).  regions: a tuple of region bit masks, one per channel: the hard Dice per
    region of the thresholded sigmoid outputs (logit > 0) instead."""
    if not logits.is_cuda:
        raise RuntimeError("dice_metric runs on the GPU only (no CPU fallback)")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    labels = labels.contiguous()
    if labels.dtype not in (torch.float32, torch.bfloat16, torch.uint8, torch.int64):
        labels = labels.long()
    ld = _channels_last_rows(logits)
    if ld == 0 or logits.data_ptr() % 16 or (ld * logits.element_size()) % 16:
        ld, logits = 0, logits.contiguous()
    _, hard = hip.seg_loss_partials(logits, labels, logits.shape[1], hip.LOSS_DICE_CE, ld, want_hard=True, regions=regions)
    return dice_from_counts(hard)
