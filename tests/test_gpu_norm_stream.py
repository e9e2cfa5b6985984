"""The InstanceNorm forward and backward-apply kernels take several rows per thread and trip: shapes at which that batching
can go wrong (fewer rows than one batch, partial last trips, channel slices of wider buffers), against float64 torch
formulas, with every output inside a sentinel-filled buffer that must come back untouched around it and fully written
inside it.  The pooled-backward and head-backward reductions, which walk rows the same way, get the same guard on small shapes.
One test states the contract of the reduce scratch these reductions share: its 256-byte header is never touched."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_kernels import _dev, check, cl, gen, ncdhw, rnd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = -32768.0          # exact in bf16, far outside every value the kernels produce here
PAD_ROWS = 3                 # sentinel rows before and after the tensor
SLOPE, EPS = 0.1, 1e-5


class Guarded:
    """a channels-last [N, *sp, C] tensor inside a sentinel-filled buffer: PAD_ROWS extra rows at either end and, unless
    layout is "dense", a second channel half (the tensor is the "first" or "second" half of 2C-wide rows)"""

    def __init__(self, N, sp, C, layout, dtype, dev):
        rows = N * sp[0] * sp[1] * sp[2]
        width = C if layout == "dense" else 2 * C
        off = C if layout == "second" else 0
        self.buf = torch.full((rows + 2 * PAD_ROWS, width), SENTINEL, dtype=dtype, device=dev)
        self.before = self.buf.clone()
        self.mask = torch.zeros(self.buf.shape, dtype=torch.bool, device=dev)
        self.mask[PAD_ROWS:PAD_ROWS + rows, off:off + C] = True
        self.t = self.buf[PAD_ROWS:PAD_ROWS + rows].view(N, *sp, width)[..., off:off + C]

    def assert_exact(self, what):
        outside = ~self.mask
        assert torch.equal(self.buf[outside], self.before[outside]), f"{what}: wrote outside its tensor"
        assert not bool((self.buf[self.mask] == SENTINEL).any()), f"{what}: left elements unwritten"


def place(t_cl, layout):
    """an input operand dense, or as the first / second half of a 2C-wide buffer (the other half holds other numbers)"""
    if layout == "dense":
        return t_cl
    C = t_cl.shape[-1]
    wide = torch.full(t_cl.shape[:-1] + (2 * C,), 5.0, dtype=t_cl.dtype, device=t_cl.device)
    v = wide[..., C:] if layout == "second" else wide[..., :C]
    v.copy_(t_cl)
    return v


@functools.lru_cache(maxsize=None)
def _reference(dtype, C, sp, res):
    """float64 forward and backward of lrelu(instance_norm(x) [+ r]) on the operands as rounded to dtype (computed once
    per case, shared by the layouts)"""
    N = 2
    x = gen(N, C, *sp, seed=1) * 2 + 0.5
    r = gen(N, C, *sp, seed=2)
    dy = gen(N, C, *sp, seed=5)
    gamma, beta = gen(C, seed=3) * 0.2 + 1, gen(C, seed=4) * 0.2
    xr, rr, dyr = (t.double() for t in rnd(dtype, x, r, dy))
    xr.requires_grad_(True); rr.requires_grad_(True)
    z = F.instance_norm(xr, weight=gamma.double(), bias=beta.double(), eps=EPS)
    if res:
        z = z + rr
    y = F.leaky_relu(z, SLOPE)
    y.backward(dyr)
    return dict(x=x, r=r, dy=dy, gamma=gamma, beta=beta, y=y.detach(), dx=xr.grad, dres=rr.grad if res else None)


@pytest.mark.parametrize("layout", ["dense", "first", "second"])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("C", [32, 48, 20, 6])
@pytest.mark.parametrize("sp", [(3, 5, 7), (8, 8, 10), (12, 12, 18)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_instnorm_act_fwd_and_bwd_apply(dtype, sp, C, res, layout):
    """res: forward with a residual, backward from the stored activation and with dres; otherwise forward without one and
    the backward recomputing the sign from x (y absent).  C = 20 takes the scalar kernels in bf16 only (20 % 4 == 0: float32
    streams 16-byte chunks); C = 6 takes them in both dtypes and in all three layouts"""
    from medicalsemseg_amd import hip
    dev = _dev()
    N = 2
    ref = _reference(dtype, C, sp, res)
    xg = place(cl(ref["x"], dtype, dev), layout)
    rg = place(cl(ref["r"], dtype, dev), layout) if res else None
    dyg = place(cl(ref["dy"], dtype, dev), layout)
    gamma, beta = ref["gamma"].to(dev), ref["beta"].to(dev)
    stats = hip.channel_stats(xg)
    a = Guarded(N, sp, C, layout, dtype, dev)
    hip.instnorm_act_fwd(xg, stats, gamma, beta, a.t, SLOPE, EPS, rg)
    a.assert_exact("instnorm fwd")
    check(ncdhw(a.t), ref["y"], dtype, "instnorm fwd")
    y_in = a.t if res else None
    red = hip.instnorm_act_bwd_reduce(xg, stats, gamma, y_in, dyg, SLOPE, EPS, None, None, False, beta)
    dx = Guarded(N, sp, C, layout, dtype, dev)
    dres = Guarded(N, sp, C, layout, dtype, dev) if res else None
    hip.instnorm_act_bwd_apply(xg, stats, gamma, y_in, dyg, red, dx.t, SLOPE, EPS, dres.t if res else None, beta)
    dx.assert_exact("instnorm dx")
    check(ncdhw(dx.t), ref["dx"], dtype, "instnorm dx", scale=float(ref["dx"].abs().max()))
    if res:
        dres.assert_exact("instnorm dres")
        check(ncdhw(dres.t), ref["dres"], dtype, "instnorm dres")


def _scratch_users(dtype, C, dev):
    """every output of one round of the reductions that work in hip.scratch: N = 2, (3, 5, 7) voxels, C channels"""
    from medicalsemseg_amd import hip
    N, sp = 2, (3, 5, 7)
    x = cl(gen(N, C, *sp, seed=61) * 2 + 0.5, dtype, dev)
    dy = cl(gen(N, C, *sp, seed=62), dtype, dev)
    gamma, beta = (gen(C, seed=63) * 0.2 + 1).to(dev), (gen(C, seed=64) * 0.2).to(dev)

    def unwritten(*shape):   # NaN never compares equal: an element a kernel leaves alone fails the comparison of the rounds
        return torch.full(shape, float("nan"), device=dev)

    out = {}
    out["channel_stats"] = hip.channel_stats(x, unwritten(N, C, 2))
    out["channel_sum"] = hip.channel_sum(x, unwritten(C))
    out["in dgamma"], out["in dbeta"] = unwritten(C), unwritten(C)
    out["in red"] = hip.instnorm_act_bwd_reduce(x, out["channel_stats"], gamma, None, dy, SLOPE, EPS, out["in dgamma"],
                                                out["in dbeta"], False, beta)
    rows, drows = x.view(N * 3 * 5 * 7, C), dy.view(N * 3 * 5 * 7, C)   # the same tensor as [210, C] token rows
    out["ln y"], out["ln dx"] = torch.empty_like(rows), torch.empty_like(rows)
    out["ln mean"], out["ln rstd"] = hip.layernorm_fwd(rows, gamma, beta, out["ln y"], EPS)
    out["ln dgamma"], out["ln dbeta"] = unwritten(C), unwritten(C)
    hip.layernorm_bwd(rows, gamma, out["ln mean"], out["ln rstd"], drows, out["ln dx"], out["ln dgamma"], out["ln dbeta"])
    if dtype == torch.bfloat16:   # statistics from the conv epilogue: partial rows per workgroup, the same second launch
        cin = cout = 32
        xc = cl(gen(N, cin, 8, 8, 8, seed=65), dtype, dev)
        w = gen(cout, cin, 3, 3, 3, seed=66, scale=(cin * 27) ** -0.5)
        wp = hip.pack_conv_k3(w.to(dev), dtype, vol=(N, 8, 8, 8))
        out["conv y"] = torch.empty(N, 8, 8, 8, cout, dtype=dtype, device=dev)
        out["conv stats"] = unwritten(N, cout, 2)
        hip.conv3d_k3(xc, wp, gen(cout, seed=67).to(dev), out["conv y"], cin, cout, out["conv stats"])
    return out


@pytest.mark.parametrize("C", [32, 6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_scratch_header_is_neither_read_nor_written(dtype, C):
    """include/msseg.h: the first 256 bytes of the reduce scratch are reserved, no kernel reads or writes them, and the
    scratch needs no initialisation.  The reductions give the same bits with the header as allocated and with every header
    byte 0xFF, and leave those bytes as they found them."""
    from medicalsemseg_amd import hip
    dev = _dev()
    header = hip.scratch(dev)[:256]
    try:
        first = _scratch_users(dtype, C, dev)
        header.fill_(0xFF)
        second = _scratch_users(dtype, C, dev)
        assert first.keys() == second.keys()
        for name in first:
            assert torch.equal(first[name], second[name]), f"{name}: depends on the scratch header"
        assert bool((header == 0xFF).all()), "a kernel wrote into the scratch header"
    finally:
        header.zero_()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,C", [((2, 6, 10, 14), 32), ((1, 4, 4, 6), 48), ((1, 2, 2, 2), 8)])
def test_instnorm_act_poolbwd_reduce_shapes(dtype, shape, C):
    """test_instnorm_act_poolbwd_reduce_equals_two_kernels' assertions on further shapes, the gradient tensor written into
    the second half of a sentinel-guarded buffer"""
    from medicalsemseg_amd import hip
    DEV = _dev()
    N, D, H, W = shape
    torch.manual_seed(12)
    y = torch.randn(N, D, H, W, C, device=DEV).to(dtype)
    gamma = torch.randn(C, device=DEV)
    beta = torch.randn(C, device=DEV) * 0.3
    stats = hip.channel_stats(y)
    a = torch.empty_like(y)
    pooled = torch.empty(N, D // 2, H // 2, W // 2, C, device=DEV, dtype=dtype)
    hip.instnorm_act_pool_fwd(y, stats, gamma, beta, a, pooled, 0.1)
    dcat = torch.randn(N, D, H, W, 2 * C, device=DEV).to(dtype)
    g = torch.randn_like(pooled)
    g_before = g.clone()
    ref_cat = dcat.clone()
    hip.maxpool2_bwd(a, g, ref_cat[..., :C], accumulate=True)
    dg_ref, db_ref = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx_ref = torch.empty_like(y)
    red_ref = hip.instnorm_act_bwd(y, stats, gamma, None, ref_cat[..., :C], dx_ref, 0.1, 1e-5, None, dg_ref, db_ref, False, beta)
    da = Guarded(N, (D, H, W), C, "second", dtype, DEV)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    red = hip.instnorm_act_poolbwd_reduce(y, stats, gamma, beta, dcat[..., :C], g, da.t, 0.1, 1e-5, dg, db, False)
    da.assert_exact("poolbwd da")
    assert torch.equal(g, g_before)
    assert torch.equal(da.t.contiguous(), ref_cat[..., :C].contiguous())
    scale = float(red_ref.abs().max())
    assert float((red - red_ref).abs().max()) < 1e-5 * scale + 1e-6
    assert float((dg - dg_ref).abs().max()) < 1e-5 * float(dg_ref.abs().max()) + 1e-6
    assert float((db - db_ref).abs().max()) < 1e-5 * float(db_ref.abs().max()) + 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3d_k1_head_dgrad_inbwd_small(dtype):
    """test_conv3d_k1_head_dgrad_inbwd's assertions at 2 x (3, 5, 7) voxels, cin 32, cout 3: fewer rows per block than the
    block has row slots, let alone one unrolled trip of the row loop; the input gradient written into a sentinel-guarded buffer"""
    from medicalsemseg_amd import hip
    DEV = _dev()
    cin, cout = 32, 3
    N, sp = 2, (3, 5, 7)
    yraw = gen(N, cin, *sp, seed=41)
    dl = gen(N, cout, *sp, seed=42)
    w = gen(cout, cin, seed=43, scale=0.2)
    gamma, beta = gen(cin, seed=44) * 0.3 + 1.0, gen(cin, seed=45) * 0.3
    yr, dlr, wr = rnd(dtype, yraw, dl, w)
    da = torch.einsum("nkdhw,kc->ncdhw", dlr, wr)
    da = rnd(dtype, da)
    mean = yr.mean(dim=(2, 3, 4), keepdim=True)
    var = (yr * yr).mean(dim=(2, 3, 4), keepdim=True) - mean * mean
    rstd = torch.rsqrt(var.clamp_min(0) + 1e-5)
    z = (yr - mean) * rstd * gamma.view(1, -1, 1, 1, 1) + beta.view(1, -1, 1, 1, 1)
    dz = torch.where(z > 0, da, da * 0.1)
    red_ref = torch.stack([dz.sum(dim=(2, 3, 4)), (dz * (yr - mean) * rstd).sum(dim=(2, 3, 4))], dim=-1)
    yc = cl(yraw, dtype, DEV)
    dlc = torch.zeros(N, *sp, 8, device=DEV, dtype=dtype)
    dlc[..., :cout] = cl(dl, dtype, DEV)
    dlc_before = dlc.clone()
    stats = hip.channel_stats(yc)
    dx = Guarded(N, sp, cin, "first", dtype, DEV)
    dg, db = torch.zeros(cin, device=DEV), torch.zeros(cin, device=DEV)
    red = hip.conv3d_k1_head_bwd_fused(dlc, w.to(DEV), dx.t, cin, cout, yc, stats, gamma.to(DEV), beta.to(DEV), 0.1, 1e-5,
                                       dgamma=dg, dbeta=db, accumulate=False)
    dx.assert_exact("head dgrad")
    assert torch.equal(dlc, dlc_before)
    check(ncdhw(dx.t), da, dtype, "head dgrad")
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    sc = float(red_ref.abs().max())
    assert float((red.cpu() - red_ref).abs().max()) / sc < tol
    assert float((db.cpu() - red_ref[..., 0].sum(0)).abs().max()) / sc < tol
    assert float((dg.cpu() - red_ref[..., 1].sum(0)).abs().max()) / sc < tol
