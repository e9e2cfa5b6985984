"""Checker for the fused AdamW step and the gradient-norm reduction: torch's documented AdamW restated in float64, the
error bounds the fp32 kernels are held to, and an fp32 emulation that shows on the CPU that a correct fp32 implementation
stays inside those bounds.

One step on (p, g, m, v) at step count t, with g multiplied by gscale first:

    p_dec = p * (1 - lr*wd)            on the elements of the decay mask (mask None: all of them)
    m'    = b1*m + (1 - b1)*g
    v'    = b2*v + (1 - b2)*g*g
    p'    = p_dec - lr/(1 - b1^t) * m' / (sqrt(v')/sqrt(1 - b2^t) + eps)

Every hyper-parameter enters as the fp32 value the kernel receives (a C float argument, or an fp32 device scalar).  torch
multiplies an fp32 parameter by the Python double 1 - lr*wd, which the multiplication rounds to fp32; round_decay_to_fp32
does the same.  At the production values lr = 4e-4, wd = 1e-5 that multiplier is exactly 1.0f: lr*wd = 4e-9 is below
2^-25, half the spacing of the floats under 1.  Decay is the identity there, in torch and in the kernel alike.

Bounds against this reference (fp32 rounding analysis with room for a device powf / sqrtf / division of a few ulp):

    |m' - ref| <= B_m = 2^-21 * (|b1*m| + |(1-b1)*g|)
    |v' - ref| <= 2^-20 * ref
    |p' - ref| <= 4 * 2^-23 * |ref| + 4e-5 * |ref - p_dec| + lr/(1 - b1^t) * B_m / denom       (step_bounds()["p"])
    after t chained steps: |p - ref| <= t * (4 * 2^-23 * |p| + 4e-5 * lr_max)   (cumulative_bound)

The last term of the p bound is B_m carried through the update.  b1*m and (1-b1)*g may cancel, and then the rounding error
of m' (three roundings of 2^-24 on the size of the terms, not of their sum) is neither small against |p'| nor against the
update |ref - p_dec|.  Among a few thousand elements the first two terms ("p_issue") hide this; among the 4.2 million of
the grid-stride case they do not: the emulation reaches 0.69 of the two-term bound there (t = 2, lr = 1e-2, gscale = 0.37)
and 0.23 of the three-term bound.  The cumulative bound needs no such term: along one gradient sequence
|m| / sqrt(v) stays of order one, so B_m / denom is a few times 2^-21, far below 4e-5.

Measured on the CPU with adamw_step_f32_emulation (tests/test_optim_host.py asserts every ratio below 0.5), 20 chained
steps from zero moments at n = 4099, worst ratio error / bound for HYPER_SETS in turn:
    per-step p  0.123 0.221 0.235,  m  0.287 0.287 0.287,  v  0.224 0.224 0.229,  cumulative  0.117 0.139 0.201

The gradient norm: sumsq_kernel adds x*x serially per thread, then over a wave (6 shuffle steps), then the 4 waves of the
block; sumsq_finalize_kernel adds the block partials serially per thread, then in a 256-wide tree (8 steps).  All terms
are non-negative, so to first order the relative error is at most (number of roundings on the longest path) * 2^-24.
"""
import math

import numpy as np
import torch

U23, U24 = 2.0 ** -23, 2.0 ** -24

# (lr, wd, b1, b2, eps) of the host emulation test
HYPER_SETS = [(4e-4, 1e-5, 0.9, 0.95, 1e-6), (1e-2, 0.05, 0.9, 0.95, 1e-6), (1e-3, 1e-2, 0.9, 0.999, 1e-8)]


def f32(x):
    """the value of a Python float once it has passed through a C float argument"""
    return float(np.float32(x))


def make_inputs(n, t, seed=0):
    """fp32 (p, g, m, v) of the kernel tests: p ~ N(0,1); g = N(0,1) * 10^U(-6,2) per element with a slice of exact zeros;
    for t > 1 a random first moment of the gradient's size and a second moment that is at least its square (as the running
    averages of one gradient sequence are), zeros for t = 1"""
    gen = torch.Generator().manual_seed(1000 + seed)
    p = torch.randn(n, generator=gen)
    scale = 10.0 ** (torch.rand(n, generator=gen) * 8 - 6)
    g = torch.randn(n, generator=gen) * scale
    z0 = n // 3
    g[z0:z0 + max(1, n // 8)] = 0.0
    if t > 1:
        m = torch.randn(n, generator=gen) * scale
        v = m * m + (torch.randn(n, generator=gen) * scale) ** 2
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v


def random_mask(n, seed=0):
    """decay mask bytes from {0, 1, 255}: the 4-byte words the vector path reads mix decayed and undecayed elements"""
    gen = torch.Generator().manual_seed(2000 + seed)
    return torch.tensor([0, 1, 255], dtype=torch.uint8)[torch.randint(0, 3, (n,), generator=gen)]


def adamw_step_f64(p, g, m, v, mask, lr, b1, b2, eps, wd, t, gscale=1.0, round_decay_to_fp32=True):
    """one AdamW step in float64 -> (p', m', v', p_dec); tensors of any float dtype, mask: None or anything that
    converts to bool per element"""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    lr, b1, b2, eps, wd, gscale = (f32(x) for x in (lr, b1, b2, eps, wd, gscale))
    mult = 1.0 - lr * wd
    if round_decay_to_fp32:
        mult = f32(mult)
    g = g * gscale
    p_dec = p * mult if mask is None else torch.where(mask.bool(), p * mult, p)
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    denom = v2.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    p2 = p_dec - lr / (1.0 - b1 ** t) * (m2 / denom)
    return p2, m2, v2, p_dec


def adamw_step_f32_emulation(p, g, m, v, mask, lr, b1, b2, eps, wd, t, gscale=1.0):
    """the same step in fp32, one rounding per operation, in the kernel's operation order (numpy float32 throughout)
    -> fp32 tensors (p', m', v')"""
    F = np.float32
    p, g, m, v = (x.numpy().astype(F) for x in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (F(x) for x in (lr, b1, b2, eps, wd, gscale))
    one = F(1.0)
    bc1 = F(one - F(np.power(b1, F(t))))
    bc2_sqrt = F(np.sqrt(F(one - F(np.power(b2, F(t))))))
    ge = g * gs
    dec = p * F(one - F(lr * wd))
    pe = dec if mask is None else np.where(mask.bool().numpy(), dec, p)
    me = b1 * m + F(one - b1) * ge
    ve = b2 * v + F(one - b2) * ge * ge
    denom = np.sqrt(ve) / bc2_sqrt + eps
    pn = pe - F(lr / bc1) * (me / denom)
    for a in (pn, me, ve):
        assert a.dtype == F
    return torch.from_numpy(pn), torch.from_numpy(me), torch.from_numpy(ve)


def step_bounds(ref, m, g, lr, b1, b2, eps, t, gscale=1.0):
    """element-wise bounds on |p' - ref|, |m' - ref|, |v' - ref| for ref = adamw_step_f64(...) on first moment m, gradient g"""
    p2, m2, v2, p_dec = ref
    lr, b1, b2, eps, gscale = (f32(x) for x in (lr, b1, b2, eps, gscale))
    bm = 2.0 ** -21 * ((b1 * m.double()).abs() + ((1.0 - b1) * gscale * g.double()).abs())
    denom = v2.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    return {"p": 4 * U23 * p2.abs() + 4e-5 * (p2 - p_dec).abs() + lr / (1.0 - b1 ** t) * bm / denom,
            "p_issue": 4 * U23 * p2.abs() + 4e-5 * (p2 - p_dec).abs(),
            "m": bm,
            "v": 2.0 ** -20 * v2}


def cumulative_bound(p_ref, t, lr_max):
    """bound on |p - p_ref| after t chained steps at learning rates up to lr_max"""
    return t * (4 * U23 * p_ref.double().abs() + 4e-5 * lr_max)


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound; an element with bound 0 must be exact (ratio 0, else inf)"""
    err = (got.double() - ref.double()).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).double())
    return float(r.max())


def sumsq_nblk(n, num_cus, n_partials):
    """blocks msseg_sumsq launches: one per 4096 elements, at most 16 per CU, at most one per entry of the partials buffer"""
    return max(1, min(-(-n // 4096), num_cus * 16, n_partials))


def sumsq_bound(n, nblk):
    """relative error bound of the summation tree: per-thread serial length + the squaring + 6 wave steps + the 4-wave add
    (2) + the finalise's serial part + its 8 tree steps, each one rounding of 2^-24"""
    k = -(-n // (nblk * 256)) + 1 + 6 + 2 + -(-nblk // 256) + 8
    return k * U24
