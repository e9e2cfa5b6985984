"""CPU tests of tests/unet_step_ref.py, the float64 references behind tests/test_gpu_unet_step_ops.py, and of
the method itself, in the manner of tests/test_conv_exact_method.py.

1. The reference ops, chained without any rounding into a whole UNet step, equal float64 autograd through the oracle's BasicUNet.
2. On the same net with emulated bf16 storage, seven errors of the kind the backward's hand-offs have had are seeded into ONE op
   each.  Every one fails that op's gate (the per-op check sees it); the whole-net comparison against the fp32 oracle, at the
   gates tests/test_gpu_kernels.py::test_unet_small_fwd_bwd uses (rel-L2 < 8e-2, < 0.6 per parameter), does not -- where it does,
   the case's entry in SEEDED says so."""
import pytest
import torch

from oracle.blocks import BasicUNet
from oracle.losses import dice_ce_loss
from tests import unet_step_ref as R

FEATURES = (16, 16, 32, 64, 128, 16)
SLOPE = 0.1
# 16 x 16 x 32, not 16^3: at 16^3 the bottom level is one voxel per channel, which torch's instance_norm (the oracle) refuses
# ("Expected more than 1 spatial element"); this is the smallest grid of the net that the oracle runs
GRID = (16, 16, 32)
WHOLE_NET_GATE, PER_PARAM_GATE = 8e-2, 0.6


def _labels(n, seed, grid):
    g = torch.Generator().manual_seed(seed)
    y = torch.zeros(n, 1, *grid)
    for b in range(n):
        lo = [int(torch.randint(0, s // 3, (1,), generator=g)) for s in grid]
        y[b, 0, lo[0]:lo[0] + grid[0] // 2, lo[1]:lo[1] + grid[1] // 2, lo[2]:lo[2] + grid[2] // 2] = 1
    return y


def _setup(n, seed=0, grid=GRID):
    torch.manual_seed(seed)
    ref = BasicUNet(1, 2, FEATURES, slope=SLOPE)
    with torch.no_grad():      # affine parameters and biases away from their (1, 0) initial values
        for name, p in ref.named_parameters():
            if ".N." in name:
                p.add_(0.2 * torch.randn_like(p))
    x = torch.randn(n, 1, *grid, generator=torch.Generator().manual_seed(seed + 1))
    return ref, x, _labels(n, seed + 2, grid)


def _oracle_step(ref, x, y, dtype):
    """(logits, dlogits, {name: grad}) of the oracle in `dtype`"""
    m = BasicUNet(1, 2, FEATURES, slope=SLOPE).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in ref.state_dict().items()})
    out = m(x.to(dtype))
    out.retain_grad()
    dice_ce_loss(out, y).backward()
    return out.detach(), out.grad.detach(), {k: p.grad.detach() for k, p in m.named_parameters()}


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _before_norm(name):
    return name.endswith(".conv.bias") and "final" not in name       # ".conv.bias": not the transposed convs' "deconv.bias"


def test_chained_reference_equals_float64_autograd():
    """features (16,16,32,64,128,16), 1 -> 2 classes, 1 x 16 x 16 x 32, no rounding anywhere: logits and every parameter
    gradient within 1e-10 of the tensor's maximum; biases in front of InstanceNorm (true gradient 0) within 1e-10 of the weight
    gradient's maximum.  The gradient of the loss with respect to the logits is taken from the oracle: the loss is no op of
    layers.py."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref, x, y = _setup(1)
    out, dout, grads = _oracle_step(ref, x, y, torch.float64)
    step = R.Step({k: v.detach() for k, v in ref.named_parameters()}, slope=SLOPE)
    logits = step.forward(_cl(x))
    assert float((logits - _cl(out)).abs().max()) <= 1e-10 * float(out.abs().max())
    got = step.backward(_cl(dout))
    assert set(got) == set(grads)
    for name, g in grads.items():
        err = float((got[name].reshape(g.shape) - g).abs().max())
        if _before_norm(name):
            wmax = float(grads[name[:-4] + "weight"].abs().max())
            assert float(got[name].abs().max()) <= 1e-10 * wmax and float(g.abs().max()) <= 1e-10 * wmax, name
        else:
            assert err <= 1e-10 * float(g.abs().max()), (name, err)
    # the unrounded chain passes its own gates trivially: the checker runs on it end to end
    assert max(step.check().values()) <= 1.0


# ---- the seeded errors -------------------------------------------------------------------------------------------------------
UNIT = "upcat_1.convs.conv_1"          # the last unit (full grid, 16 channels): its sums come from the head's backward
DEC0 = "upcat_1.convs.conv_0"          # its first conv's input is cat([skip | up])


def _norm_parts(ops, sign_from=None):
    y, st, da, ga, be = ops
    return R.norm_bwd_parts(y, st, da, ga, be, SLOPE, 1e-5, sign_from)


def _from_red(dz, xhat, sc, red):
    return [R.norm_bwd_apply_parts(dz, xhat, sc, red), red, red[..., 1].sum(0), red[..., 0].sum(0)]


def _red_tile_missing(kind, where, ops, outs):
    if kind == "norm_act_bwd" and where == UNIT:
        dz, xhat, sc = _norm_parts(ops)
        red = outs[1].clone()
        red[1] -= R.norm_bwd_red(dz[1:2, 4:8, 8:12], xhat[1:2, 4:8, 8:12])[0]      # one 4 x 4 x 16 tile of sample 1
        return _from_red(dz, xhat, sc, red)


def _red_wrong_sample_rstd(kind, where, ops, outs):
    if kind == "norm_act_bwd" and where == UNIT:
        dz, xhat, sc = _norm_parts(ops)
        _, rstd = R.mean_rstd(ops[1], 32 ** 3, 1e-5)
        red = outs[1].clone()
        red[..., 1] = red[..., 1] * (rstd.flip(0) / rstd).reshape(2, -1)         # xhat formed with the other sample's rstd
        return _from_red(dz, xhat, sc, red)


def _sign_from_da(kind, where, ops, outs):
    if kind == "norm_act_bwd" and where == UNIT:
        dz, xhat, sc = _norm_parts(ops, sign_from=ops[2])
        return _from_red(dz, xhat, sc, R.norm_bwd_red(dz, xhat))


def _halves_swapped(kind, where, ops, outs):
    if kind == "conv3_dgrad_split" and where == DEC0:
        return [outs[1], outs[0]]


def _dbeta_twice(kind, where, ops, outs):
    if kind == "norm_act_bwd" and where == UNIT:
        return [outs[0], outs[1], outs[2], 2 * outs[3]]


def _dbias_7_of_8(kind, where, ops, outs):
    if kind == "deconv_bwd" and where == "upcat_1":
        dy = ops[1]
        return [outs[0], outs[1], outs[2] - R.channel_sum(dy[:, 1::2, 1::2, 1::2])]


def _pool_last_tie(kind, where, ops, outs):
    if kind == "pool_skip_grad" and where == "conv_0":
        act, skip, g = ops
        ties = (R.maxpool_bwd(act, torch.ones_like(g)) != R.maxpool_bwd(act, torch.ones_like(g), last=True)).any()
        assert bool(ties), "no tied maximum in the stored activation: the case does not exercise the convention"
        return [R.pool_skip_grad(act, skip, g, last=True)]


# name: (tamper, op kind whose gate must fail, the parameter it damages most directly,
#        does the whole-net comparison miss it (both existing gates hold)?)
SEEDED = {
    "red misses one 4x4x16 tile of one sample": (_red_tile_missing, "norm_act_bwd", UNIT + ".adn.N.bias", True),
    "red's second sum with the other sample's rstd": (_red_wrong_sample_rstd, "norm_act_bwd", UNIT + ".adn.N.weight", True),
    # (ii) does NOT hold for the next three on this net: seeded into the LAST unit, whose gradients are the largest of the net,
    # they move the whole-net norm over its gate too (measured: 1.6e-1, 9.4e-2 and 1.3e-1 against 8e-2; the doubled dbeta is a
    # relative error of exactly 1 on its parameter, and that 32-element tensor carries 1.3e-1 of the net's gradient norm)
    "LeakyReLU sign from da instead of the pre-activation": (_sign_from_da, "norm_act_bwd", UNIT + ".conv.weight", False),
    "dcat halves swapped (up first)": (_halves_swapped, "conv3_dgrad_split", "upcat_1.upsample.deconv.weight", False),
    "dbeta of one unit accumulated twice": (_dbeta_twice, "norm_act_bwd", UNIT + ".adn.N.bias", False),
    "deconv bias gradient over 7 of the 8 child positions": (_dbias_7_of_8, "deconv_bwd", "upcat_1.upsample.deconv.bias", True),
    "max-pool gradient to the last tied maximum": (_pool_last_tie, "pool_skip_grad", "conv_0.conv_1.adn.N.bias", True),
}


@pytest.fixture(scope="module")
def bf16_case():
    """the 16-wide net at 2 x 32^3 (the wrong-sample error needs a second sample; at 16 x 16 x 32 the 16-voxel level's dgamma
    already misses the 0.6 per-parameter gate with nothing seeded) in emulated bf16 storage: the forward and the loss, run
    once -- every seeded error sits in the backward -- and the fp32 oracle's gradients"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ref, x, y = _setup(2, grid=(32, 32, 32))
    out, dout, grads = _oracle_step(ref, x, y, torch.float32)
    step = R.Step({k: v.detach() for k, v in ref.named_parameters()}, slope=SLOPE, store=torch.bfloat16)
    logits = step.forward(_cl(x)).float().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    dice_ce_loss(logits, y).backward()             # the loss on the stored logits, as the step's loss kernel sees them
    return step, len(step.log), _cl(logits.grad), grads


def _whole_net(got, grads):
    num = den = 0.0
    per = {}
    for name, g in grads.items():
        if _before_norm(name):
            continue
        d2, r2 = float(((got[name].reshape(g.shape) - g.double()) ** 2).sum()), float((g.double() ** 2).sum())
        num, den = num + d2, den + r2
        per[name] = (d2 / (r2 + 1e-30)) ** 0.5
    return (num / den) ** 0.5, per


def _run(bf16_case, tamper):
    step, nfwd, dl, grads = bf16_case
    del step.log[nfwd:]
    step.grads, step.tamper = {}, tamper
    got = step.backward(dl)
    return step, nfwd, _whole_net(got, grads)


def test_emulated_bf16_step_passes_every_gate(bf16_case):
    step, nfwd, (tot, per) = _run(bf16_case, None)
    worst = step.check()
    print("emulated bf16 step, worst error / gate per op kind:", {k: round(v, 3) for k, v in worst.items()},
          f"whole-net rel-L2 {tot:.3e}, worst parameter {max(per.items(), key=lambda kv: kv[1])}")
    assert max(worst.values()) <= 1.0
    assert tot < WHOLE_NET_GATE and max(per.values()) < PER_PARAM_GATE


@pytest.mark.parametrize("name", list(SEEDED))
def test_seeded_error_fails_its_op_gate_and_hides_in_the_whole_net_norm(bf16_case, name):
    tamper, kind, param, hidden = SEEDED[name]
    step, nfwd, (tot, per) = _run(bf16_case, tamper)
    print(f"{name}: whole-net rel-L2 {tot:.3e} (gate {WHOLE_NET_GATE}), {param} {per[param]:.3e}, worst parameter "
          f"{max(per.items(), key=lambda kv: kv[1])} (gate {PER_PARAM_GATE})")
    with pytest.raises(R.GateError, match=kind):
        step.check(first=nfwd)                                               # (i) the per-op gate sees it
    assert (tot < WHOLE_NET_GATE and max(per.values()) < PER_PARAM_GATE) == hidden     # (ii) the existing whole-net gates
