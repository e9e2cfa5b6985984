"""Two places where the backward no longer writes a full-resolution tensor for the next kernel to read back.

The stem weight gradient applies the InstanceNorm + LeakyReLU backward while it loads its operand (conv3d_stem_wgrad_inbwd):
its dW must have the bits of the two-kernel path it replaces (backward apply into a tensor, then the stem weight gradient), on
whole and ragged tiles, one tile per sample, channel slices of wider rows, with and without the affine parameters and
accumulation, and must match a float64 gradient.

The head backward leaves its input gradient unstored (conv3d_k1_head_bwd_fused with da None) and the backward apply of the
unit in front of the head forms it again (instnorm_act_bwd_apply_head): same sums and weight gradient, and the dy of the plain
apply fed with the stored gradient, bit for bit.

Both in a whole UNet training step, against the routes they replace."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_kernels import _dev, check, cl, gen, ncdhw, rnd
from tests.test_gpu_norm_stream import Guarded, place

pytestmark = pytest.mark.gpu

SLOPE, EPS = 0.1, 1e-5
BF16 = torch.bfloat16

# whole tiles (4 x 4 x 16); partial tiles in all three axes; one tile per sample (the constants change at every tile); ragged
# tiles with three samples
STEM_GRIDS = [(2, (8, 8, 16)), (1, (5, 6, 18)), (3, (4, 4, 16)), (2, (9, 14, 35))]


@functools.lru_cache(maxsize=None)
def _stem_case(cout, N, sp, affine):
    """operands (as rounded to bf16) of one stem unit's backward and its float64 result: the backward sums `red` of the
    InstanceNorm + LeakyReLU backward and the weight gradient of the one-channel 3x3x3 conv in front of it"""
    x = gen(N, 1, *sp, seed=1)
    yraw = gen(N, cout, *sp, seed=2) * 1.5 + 0.3
    da = gen(N, cout, *sp, seed=3)
    gamma = (gen(cout, seed=4) * 0.2 + 1) if affine else None
    beta = (gen(cout, seed=5) * 0.2) if affine else None
    xr, yr, dar = (t.double() for t in rnd(BF16, x, yraw, da))
    yr.requires_grad_(True)
    z = F.instance_norm(yr, weight=gamma.double() if affine else None, bias=beta.double() if affine else None, eps=EPS)
    F.leaky_relu(z, SLOPE).backward(dar)
    dy = yr.grad
    w = torch.zeros(cout, 1, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(xr, w, padding=1).backward(dy)
    with torch.no_grad():
        mean = yr.mean(dim=(2, 3, 4), keepdim=True)
        var = (yr * yr).mean(dim=(2, 3, 4), keepdim=True) - mean * mean
        xh = (yr - mean) * torch.rsqrt(var.clamp_min(0) + EPS)
        dz = torch.where(z > 0, dar, dar * SLOPE)
        red = torch.stack([dz.sum(dim=(2, 3, 4)), (dz * xh).sum(dim=(2, 3, 4))], dim=-1).float()
    return dict(x=x, yraw=yraw, da=da, gamma=gamma, beta=beta, red=red, dw=w.grad)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("layout", ["dense", "first", "second"])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("N,sp", STEM_GRIDS)
@pytest.mark.parametrize("cout", [32, 64, 48])
def test_stem_wgrad_inbwd(cout, N, sp, affine, layout, acc):
    from medicalsemseg_amd import hip
    dev = _dev()
    ref = _stem_case(cout, N, sp, affine)
    xg = cl(ref["x"], BF16, dev)
    yg = place(cl(ref["yraw"], BF16, dev), layout)
    dag = place(cl(ref["da"], BF16, dev), layout)
    gamma = ref["gamma"].to(dev) if affine else None
    beta = ref["beta"].to(dev) if affine else None
    stats = hip.channel_stats(yg)
    S = sp[0] * sp[1] * sp[2]
    dw0 = gen(cout, 1, 3, 3, 3, seed=7).to(dev) if acc else torch.full((cout, 1, 3, 3, 3), float("nan"), device=dev)

    def two_kernels(red):
        dy = torch.empty(N, *sp, cout, dtype=BF16, device=dev)
        hip.instnorm_act_bwd_apply(yg, stats, gamma, None, dag, red, dy, SLOPE, EPS, None, beta)
        dw = dw0.clone()
        hip.conv3d_gather_wgrad(xg, dy, dw, 1, cout, 3, 1, 1, acc)
        return dw

    def fused(red):
        dw = dw0.clone()
        hip.conv3d_stem_wgrad_inbwd(xg, yg, dag, stats, red, gamma, beta, SLOPE, EPS, dw, cout, 3, acc)
        return dw

    # an arbitrary red: the bits of the two-kernel path
    red_any = (gen(N, cout, 2, seed=6) * (0.2 * S)).to(dev)
    assert torch.equal(fused(red_any), two_kernels(red_any)), "stem wgrad: not the two-kernel path's bits"
    # the true sums: the float64 gradient (and again the two-kernel path's bits)
    red = ref["red"].to(dev)
    dw = fused(red)
    assert torch.equal(dw, two_kernels(red)), "stem wgrad: not the two-kernel path's bits (true sums)"
    got = dw - dw0 if acc else dw
    check(got.cpu(), ref["dw"], BF16, "stem wgrad")


def test_stem_wgrad_inbwd_refuses():
    """ineligible operands are an error, not another path"""
    from medicalsemseg_amd import hip
    dev = _dev()
    N, sp, cout = 1, (4, 4, 16), 40
    x = torch.zeros(N, *sp, 1, dtype=BF16, device=dev)
    y = torch.zeros(N, *sp, cout, dtype=BF16, device=dev)
    stats = torch.zeros(N, cout, 2, device=dev)
    dw = torch.zeros(cout, 1, 3, 3, 3, device=dev)
    with pytest.raises(RuntimeError):
        hip.conv3d_stem_wgrad_inbwd(x, y, y, stats, stats, None, None, SLOPE, EPS, dw, cout, 3, False)


HEAD_GRIDS = [(1, (2, 3, 5)), (2, (4, 6, 10)), (2, (8, 8, 16))]   # the first: fewer rows than one batch of four


@functools.lru_cache(maxsize=None)
def _head_case(dtype, cin, cout, N, sp, affine):
    """operands of the head backward and the float64 dy of the unit in front of it, from the head's input gradient as rounded
    to dtype"""
    yraw = gen(N, cin, *sp, seed=41)
    dl = gen(N, cout, *sp, seed=42)
    w = gen(cout, cin, seed=43, scale=0.2)
    gamma = (gen(cin, seed=44) * 0.3 + 1.0) if affine else None
    beta = (gen(cin, seed=45) * 0.3) if affine else None
    yr, dlr, wr = rnd(dtype, yraw, dl, w)
    da = rnd(dtype, torch.einsum("nkdhw,kc->ncdhw", dlr, wr))
    y64 = yr.double().requires_grad_(True)
    z = F.instance_norm(y64, weight=gamma.double() if affine else None, bias=beta.double() if affine else None, eps=EPS)
    F.leaky_relu(z, SLOPE).backward(da.double())
    return dict(yraw=yraw, dl=dl, w=w, gamma=gamma, beta=beta, dy=y64.grad)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("N,sp", HEAD_GRIDS)
@pytest.mark.parametrize("cout", [2, 3, 4])
@pytest.mark.parametrize("cin", [16, 32, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_head_backward_without_da(dtype, cin, cout, N, sp, affine):
    from medicalsemseg_amd import hip
    dev = _dev()
    ref = _head_case(dtype, cin, cout, N, sp, affine)
    yc = cl(ref["yraw"], dtype, dev)
    ldl = 16 // yc.element_size()
    dlc = torch.zeros(N, *sp, ldl, device=dev, dtype=dtype)
    dlc[..., :cout] = cl(ref["dl"], dtype, dev)
    dlc_before = dlc.clone()
    w = ref["w"].to(dev)
    gamma = ref["gamma"].to(dev) if affine else None
    beta = ref["beta"].to(dev) if affine else None
    stats = hip.channel_stats(yc)

    def head(da):
        dw = torch.full((cout, cin), float("nan"), device=dev)
        dg = torch.full((cin,), float("nan"), device=dev) if affine else None
        db = torch.full((cin,), float("nan"), device=dev) if affine else None
        red = hip.conv3d_k1_head_bwd_fused(dlc, w, da, cin, cout, yc, stats, gamma, beta, SLOPE, EPS, dw, False, dg, db, False)
        return red, dw, dg, db

    da = torch.empty(N, *sp, cin, dtype=dtype, device=dev)
    stored, unstored = head(da), head(None)
    for name, a, b in zip(("red", "dW", "dgamma", "dbeta"), stored, unstored):        # (a)
        assert (a is None and b is None) or torch.equal(a, b), f"head backward without da: {name} differs from the storing form"
    red = stored[0]
    dy_plain = torch.empty(N, *sp, cin, dtype=dtype, device=dev)
    hip.instnorm_act_bwd_apply(yc, stats, gamma, None, da, red, dy_plain, SLOPE, EPS, None, beta)
    dy = Guarded(N, sp, cin, "second", dtype, dev)
    hip.instnorm_act_bwd_apply_head(yc, stats, gamma, beta, dlc, w, cout, red, dy.t, SLOPE, EPS)
    dy.assert_exact("apply with the head source")                                       # (b)
    assert torch.equal(dlc, dlc_before)
    assert torch.equal(dy.t.contiguous(), dy_plain), "apply with the head source: not the plain apply's bits"
    check(ncdhw(dy.t), ref["dy"], dtype, "instnorm dx", scale=float(ref["dy"].abs().max()))   # (c)


def _unet_step(monkeypatch, off):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models.unet import UNET_FEATURES, UNet
    dev = _dev()
    for k in ("MSSEG_NO_STEM_INBWD", "MSSEG_NO_HEAD_DEFER"):
        if off:
            monkeypatch.setenv(k, "1")
        else:
            monkeypatch.delenv(k, raising=False)
    torch.manual_seed(0)
    net = UNet(1, 3, UNET_FEATURES["UNet"], compute_dtype=BF16).to(dev)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 1, 32, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 3, (2, 1, 32, 32, 32), generator=g).float().to(dev)
    hip.TIMER.records.clear()
    hip.TIMER.enabled = True
    try:
        loss = DiceCELoss()(net((x, None, None)), y)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        hip.TIMER.enabled = False
    ran = set(hip.TIMER.summary())
    hip.TIMER.records.clear()
    return {n: p.grad.detach().clone() for n, p in net.named_parameters()}, ran


def test_unet_step_same_gradients_with_fused_backward(monkeypatch):
    """UNet base at 32^3, batch 2, bf16, forward + DiceCE + backward: every parameter gradient of the fused route equals the
    routes they replace (MSSEG_NO_STEM_INBWD=1, MSSEG_NO_HEAD_DEFER=1) bit for bit, and the two new entry points run exactly when
    they are not switched off"""
    g_off, ran_off = _unet_step(monkeypatch, True)
    g_on, ran_on = _unet_step(monkeypatch, False)
    for key in ("conv3d_stem_wgrad_inbwd", "instnorm_act_bwd_apply_head"):
        assert key in ran_on and key not in ran_off, (key, sorted(ran_on), sorted(ran_off))
    assert g_on.keys() == g_off.keys() and len(g_on) > 40
    for n in g_on:
        assert torch.equal(g_on[n], g_off[n]), f"gradient of {n} differs between the fused and the two-kernel backward"
