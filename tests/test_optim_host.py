"""The AdamW checker of tests/optim_ref.py against torch.optim.AdamW in float64, the decay-is-identity fact at the production
hyper-parameters, and the fp32 emulation against the bounds that the GPU tests hold the kernel to.  No GPU."""
import numpy as np
import pytest
import torch

from tests import optim_ref as R


def test_f64_step_equals_torch_adamw_float64():
    """10 steps, two param groups (wd 0.05 and 0), lr changed mid-way: the restated algorithm is torch's"""
    lr, b1, b2, eps, wd = (R.f32(x) for x in (1e-2, 0.9, 0.95, 1e-6, 0.05))
    gen = torch.Generator().manual_seed(3)
    shapes = [(7, 5), (11,)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.AdamW([{"params": [ps[0]], "weight_decay": wd}, {"params": [ps[1]], "weight_decay": 0.0}],
                            lr=lr, betas=(b1, b2), eps=eps)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    masks = [torch.ones(shapes[0], dtype=torch.uint8), torch.zeros(shapes[1], dtype=torch.uint8)]
    for t in range(1, 11):
        if t == 6:
            lr = R.f32(3e-3)
            for grp in opt.param_groups:
                grp["lr"] = lr
        gs = [torch.randn(s, generator=gen, dtype=torch.float64) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=gen))
              for s in shapes]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
        for i, g in enumerate(gs):
            p, m, v = mine[i]
            mine[i] = R.adamw_step_f64(p, g, m, v, masks[i], lr, b1, b2, eps, wd, t, 1.0, round_decay_to_fp32=False)[:3]
        for i, p in enumerate(ps):
            st = opt.state[p]
            for got, ref, what in ((mine[i][0], p.detach(), "p"), (mine[i][1], st["exp_avg"], "m"),
                                   (mine[i][2], st["exp_avg_sq"], "v")):
                err = float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())
                assert err <= 1e-12, f"step {t} group {i} {what}: relative error {err:.3e}"


def test_production_decay_multiplier_is_one_as_in_torch():
    """lr = 4e-4, wd = 1e-5: 1 - lr*wd rounds to 1.0f, and torch's fp32 AdamW step moves a decayed and an undecayed copy of
    one parameter to the same bits"""
    lr, wd = 4e-4, 1e-5
    assert np.float32(1.0 - lr * wd) == np.float32(1.0)
    assert np.float32(1.0) - np.float32(lr) * np.float32(wd) == np.float32(1.0)
    p0 = torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 3
    a, b = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([{"params": [a], "weight_decay": wd}, {"params": [b], "weight_decay": 0.0}], lr=lr,
                            betas=(0.9, 0.95), eps=1e-6)
    for _ in range(3):
        g = torch.randn(4096, generator=torch.Generator().manual_seed(2))
        a.grad, b.grad = g.clone(), g.clone()
        opt.step()
        assert torch.equal(a.detach(), b.detach())
    # the reference with the fp32 multiplier agrees; the unrounded one does decay
    q = R.adamw_step_f64(p0, g, p0 * 0, p0 * 0, None, lr, 0.9, 0.95, 1e-6, wd, 1, 1.0, True)
    assert torch.equal(q[3], p0.double())
    q = R.adamw_step_f64(p0, g, p0 * 0, p0 * 0, None, lr, 0.9, 0.95, 1e-6, wd, 1, 1.0, False)
    assert not torch.equal(q[3], p0.double())


def emulation_ratios(hyper, n=4099, steps=20):
    """worst error / bound of the fp32 emulation over `steps` chained steps: (per-step p, m, v, cumulative)"""
    lr, wd, b1, b2, eps = hyper
    mask = R.random_mask(n)
    p, _, m, v = R.make_inputs(n, 1)
    pc = p.double()
    mc, vc = m.double(), v.double()
    worst = [0.0, 0.0, 0.0, 0.0]
    for t in range(1, steps + 1):
        g = R.make_inputs(n, 1, seed=t)[1]
        gs = 1.0 if t % 2 else 0.37
        ref = R.adamw_step_f64(p, g, m, v, mask, lr, b1, b2, eps, wd, t, gs)
        bnd = R.step_bounds(ref, m, g, lr, b1, b2, eps, t, gs)
        pc, mc, vc, _ = R.adamw_step_f64(pc, g, mc, vc, mask, lr, b1, b2, eps, wd, t, gs)
        p, m, v = R.adamw_step_f32_emulation(p, g, m, v, mask, lr, b1, b2, eps, wd, t, gs)
        for i, (got, r, b) in enumerate(((p, ref[0], bnd["p"]), (m, ref[1], bnd["m"]), (v, ref[2], bnd["v"]),
                                         (p, pc, R.cumulative_bound(pc, t, R.f32(lr))))):
            worst[i] = max(worst[i], R.worst_ratio(got, r, b))
    return worst


@pytest.mark.parametrize("hyper", R.HYPER_SETS)
def test_fp32_emulation_stays_within_half_of_the_bounds(hyper):
    """a correct fp32 implementation has 2x head-room under every bound of the GPU tests (ratios: optim_ref's docstring)"""
    worst = emulation_ratios(hyper)
    print("emulation ratios (p, m, v, cumulative)", hyper, ["%.3f" % w for w in worst])
    for w, what in zip(worst, ("per-step p", "m", "v", "cumulative p")):
        assert w <= 0.5, f"{what}: emulation error is {w:.3f} of the bound at {hyper}"


@pytest.mark.parametrize("t", [1, 2, 7, 1000, 100000])
def test_fp32_emulation_single_step_from_random_state(t):
    """the single-step inputs of the GPU kernel test (random moments for t > 1), at both of its (lr, wd) pairs"""
    n = 4099
    p, g, m, v = R.make_inputs(n, t)
    mask = R.random_mask(n)
    for lr, wd in ((1e-2, 0.05), (4e-4, 1e-5)):
        for gs in (1.0, 0.37):
            ref = R.adamw_step_f64(p, g, m, v, mask, lr, 0.9, 0.95, 1e-6, wd, t, gs)
            bnd = R.step_bounds(ref, m, g, lr, 0.9, 0.95, 1e-6, t, gs)
            got = R.adamw_step_f32_emulation(p, g, m, v, mask, lr, 0.9, 0.95, 1e-6, wd, t, gs)
            for k, i in (("p", 0), ("m", 1), ("v", 2)):
                w = R.worst_ratio(got[i], ref[i], bnd[k])
                assert w <= 0.5, f"{k}: emulation error is {w:.3f} of the bound at t={t} lr={lr} gscale={gs}"


def test_fp32_emulation_grid_stride_size_needs_the_cancellation_term():
    """4.2 M elements (the grid-stride case of the GPU test on a 256-CU part), t = 2, lr = 1e-2, gscale = 0.37: among so
    many elements some have b1*m and (1-b1)*g cancel to a thousandth of their size next to a small p, and the rounding
    error of m' reaches p' through the update.  Without the propagated m bound the emulation takes more than half of the
    p bound; with it, it stays under half"""
    n = 256 * 16 * 1024 + 1028
    p, g, m, v = R.make_inputs(n, 2)
    mask = R.random_mask(n)
    ref = R.adamw_step_f64(p, g, m, v, mask, 1e-2, 0.9, 0.95, 1e-6, 0.05, 2, 0.37)
    bnd = R.step_bounds(ref, m, g, 1e-2, 0.9, 0.95, 1e-6, 2, 0.37)
    got = R.adamw_step_f32_emulation(p, g, m, v, mask, 1e-2, 0.9, 0.95, 1e-6, 0.05, 2, 0.37)
    w_issue, w = R.worst_ratio(got[0], ref[0], bnd["p_issue"]), R.worst_ratio(got[0], ref[0], bnd["p"])
    print(f"p ratio without the propagated m term {w_issue:.3f}, with it {w:.3f}")
    assert w <= 0.5


def test_sumsq_bound_terms():
    assert R.sumsq_nblk(1, 256, 4096) == 1 and R.sumsq_nblk(4097, 256, 4096) == 2
    assert R.sumsq_nblk(1_000_003, 256, 3) == 3 and R.sumsq_nblk(10 ** 9, 256, 8192) == 4096
    assert R.sumsq_bound(256, 1) == (1 + 1 + 6 + 2 + 1 + 8) * 2.0 ** -24
    assert R.sumsq_bound(1_000_003, 3) == (1303 + 1 + 6 + 2 + 1 + 8) * 2.0 ** -24
