"""Float64 references of region-based training (--label_regions): the sigmoid losses against targets
t = (mask[c] >> label) & 1, the hard counts, the decode rule and the overlap counts of two label maps.  Written from the
formulas of include/msseg.h; nothing here touches the GPU.  Logits are expected in the tested dtype's values already
(upcast, not re-drawn), so that no rounding moves a value across the `> 0` threshold between the two sides."""
import numpy as np
import torch

BRAIN_TUMOUR = ((0b1110, 0b1100, 0b1000), (1, 2, 3))          # --label_regions 1,2,3=1 2,3=2 3=3


def targets(labels, masks):
    """labels [N, 1, *sp] (any dtype) -> float64 [N, C, *sp]; a label outside 0..31 is in no region"""
    lab = labels.long()
    ok = (lab >= 0) & (lab < 32)
    sh = lab.clamp(0, 31)
    return torch.cat([(((torch.full_like(lab, int(m)) >> sh) & 1) * ok).double() for m in masks], dim=1)


def _sums(x, t):
    p = torch.sigmoid(x)
    dims = tuple(range(2, x.dim()))
    return p, (p * t).sum(dims), t.sum(dims), dims


def _bce(x, t):
    return x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))


def _focal(x, t):
    """sigmoid focal value, gamma 2: sigmoid(z)^2 * bce with z = -x * (2t - 1)"""
    z = -x * (2 * t - 1)
    return torch.exp(2 * torch.nn.functional.logsigmoid(z)) * _bce(x, t)


def _dice(p, inter, tsum, dims, snr, sdr):
    return (1 - (2 * inter + snr) / ((p * p).sum(dims) + tsum + sdr)).mean()


def region_loss(kind, x, labels, masks, snr=1e-5, sdr=1e-5, alpha=0.5, beta=0.5):
    """kind: dice_ce | tversky | dice_focal; x float64 [N, C, *sp] -> (total, first term, second term) as 0-dim tensors"""
    t = targets(labels, masks)
    p, inter, tsum, dims = _sums(x, t)
    if kind == "tversky":
        first = (1 - (inter + snr) / (inter + alpha * (p.sum(dims) - inter) + beta * (tsum - inter) + sdr)).mean()
        second = torch.zeros((), dtype=x.dtype)
    else:
        first = _dice(p, inter, tsum, dims, snr, sdr)
        second = (_bce(x, t) if kind == "dice_ce" else _focal(x, t)).mean()
    return first + second, first, second


def region_partial(kind, x, labels, masks):
    """partial [N, C, 4] = (sum p*t, sum p^2 | sum p (tversky), sum t, sum of BCE | 0 | sum of focal values)"""
    t = targets(labels, masks)
    p, inter, tsum, dims = _sums(x, t)
    slot1 = p.sum(dims) if kind == "tversky" else (p * p).sum(dims)
    slot3 = torch.zeros_like(inter) if kind == "tversky" else (_bce(x, t) if kind == "dice_ce" else _focal(x, t)).sum(dims)
    return torch.stack([inter, slot1, tsum, slot3], dim=-1)


def region_hard(x, labels, masks):
    """hard [N, C, 3] = (|P & T|, |P|, |T|) with P = (x > 0)"""
    t = targets(labels, masks)
    pm = (x > 0).double()
    dims = tuple(range(2, x.dim()))
    return torch.stack([(pm * t).sum(dims), pm.sum(dims), t.sum(dims)], dim=-1)


def loss_and_grad(kind, logits, labels, masks, scale=3.0, **kw):
    """float64 (loss triple as floats, partial, hard, gradient of scale * loss w.r.t. the logits)"""
    x = logits.double().clone().requires_grad_(True)
    total, first, second = region_loss(kind, x, labels, masks, **kw)
    (total * scale).backward()
    xd = x.detach()
    return ((float(total.detach()), float(first.detach()), float(second.detach())), region_partial(kind, xd, labels, masks),
            region_hard(xd, labels, masks), x.grad)


def decode(logits, values):
    """numpy logits [C, V] -> (uint8 map [V], uint16 bits [V]); NaN and 0 do not fire, later regions paint over earlier"""
    logits = np.asarray(logits)
    with np.errstate(invalid="ignore"):
        fired = logits > 0
    bits = np.zeros(logits.shape[1], dtype=np.uint16)
    out = np.zeros(logits.shape[1], dtype=np.uint8)
    for c in range(logits.shape[0]):
        bits |= (fired[c].astype(np.uint16) << np.uint16(c)).astype(np.uint16)
        out[fired[c]] = values[c]
    return out, bits


def lut(mask):
    return np.array([(int(mask) >> v) & 1 if v < 32 else 0 for v in range(256)], dtype=np.uint8)


def counts(pred, label, masks):
    """two uint8 maps -> float64 [R, 3] = (|P_r & T_r|, |P_r|, |T_r|)"""
    out = np.zeros((len(masks), 3), dtype=np.float64)
    for r, m in enumerate(masks):
        t = lut(m)
        p, g = t[np.asarray(pred).reshape(-1)], t[np.asarray(label).reshape(-1)]
        out[r] = (int((p & g).sum()), int(p.sum()), int(g.sum()))
    return out
