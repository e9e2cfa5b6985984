"""Checker for the Tversky and Dice + focal criteria: MONAI's definitions, as the reference constructs the two losses,
restated in plain torch.  Works in any float dtype; the GPU tests evaluate it in float64.

x: logits [N, C, *spatial]; labels [N, 1, *spatial] (integer valued); p = softmax(x, dim=1); t = one-hot(labels).
Per (n, c), over the voxels: I = sum p*t, P = sum p, P2 = sum p^2, T = sum t.

  TverskyLoss(to_onehot_y=True, softmax=True, alpha, beta, smooth_nr, smooth_dr):
      mean_{n,c} 1 - (I + smooth_nr) / (I + alpha*(P - I) + beta*(T - I) + smooth_dr)
  DiceFocalLoss(to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr, smooth_dr), gamma 2, lambdas 1:
      mean_{n,c} 1 - (2I + smooth_nr) / (P2 + T + smooth_dr)
      + mean over all N*C*S elements of the SIGMOID focal loss of the raw logits (MONAI's FocalLoss never sees the
        softmax flag): exp(gamma * logsigmoid(-x*(2t - 1))) * (x - x*t - logsigmoid(x))
"""
import torch
import torch.nn.functional as F


def _sums(logits, labels):
    n_cls = logits.shape[1]
    p = torch.softmax(logits, dim=1)
    t = F.one_hot(labels.long().squeeze(1), n_cls).movedim(-1, 1).to(p.dtype)
    red = tuple(range(2, logits.dim()))
    return p, t, red


def tversky_loss(logits, labels, alpha, beta, smooth_nr=1e-5, smooth_dr=1e-5):
    p, t, red = _sums(logits, labels)
    inter = (p * t).sum(red)
    fp = alpha * (p.sum(red) - inter)
    fn = beta * (t.sum(red) - inter)
    return (1.0 - (inter + smooth_nr) / (inter + fp + fn + smooth_dr)).mean()


def dice_focal_terms(logits, labels, smooth_nr=1e-5, smooth_dr=1e-5, gamma=2.0):
    """(dice term, focal term); the loss is their sum"""
    p, t, red = _sums(logits, labels)
    inter = (p * t).sum(red)
    dice = (1.0 - (2.0 * inter + smooth_nr) / ((p * p).sum(red) + t.sum(red) + smooth_dr)).mean()
    bce = logits - logits * t - F.logsigmoid(logits)
    weight = torch.exp(gamma * F.logsigmoid(-logits * (2.0 * t - 1.0)))
    return dice, (weight * bce).mean()


def dice_focal_loss(logits, labels, smooth_nr=1e-5, smooth_dr=1e-5):
    dice, focal = dice_focal_terms(logits, labels, smooth_nr, smooth_dr)
    return dice + focal
