"""GPU parity of FocalNetUNETR: the large depthwise Conv3d kernels (k 3..11) against stock torch-CPU fp32 convolutions (the
tolerance rule of tests/test_gpu_kernels.py) and bit-exactly on integer inputs, the focal modulation kernels against
autograd of the same expressions, the HIP encoder against the fixture the REFERENCE's own FocalNet produced, the whole net
against tests/focalnet_ref.py inside the CPU oracle's decoder, and training steps."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden_util import det_fill_, det_tensor
from tests.test_gpu_baseline import _blobs
from tests.test_gpu_kernels import DTYPES, check, cl, gen, ncdhw, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD_CFG = dict(patch_size=(2, 2, 2), in_chans=1, embed_dim=16, depths=(2, 1, 1), focal_windows=(3, 5, 3))

DW_CASES = [(3, 8, (3, 4, 5)),
            (5, 16, (2, 2, 2)),          # grid smaller than the kernel
            (7, 24, (7, 9, 13)),         # ragged, partial tiles in every axis
            (9, 48, (12, 12, 12)),
            (11, 16, (6, 6, 6)),         # the deepest production stage in miniature
            (11, 8, (1, 1, 37)),         # degenerate axes and a long W
            (9, 32, (16, 16, 16))]


def _taps(w, dtype, dev):
    C = w.shape[0]
    return w.reshape(C, -1).t().contiguous().to(dev, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,C,sp", DW_CASES)
def test_dwconv_large(dtype, K, C, sp):
    from medicalsemseg_amd import hip, ops
    dev = torch.device(DEV)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    N = 2
    x = gen(N, C, *sp, seed=1)
    w = gen(C, 1, K, K, K, seed=2, scale=float(K) ** -1.5)
    dy = gen(N, C, *sp, seed=4)
    xr, wr, dyr = rnd(dtype, x, w, dy)
    xr.requires_grad_(True); wr.requires_grad_(True)
    yref = F.conv3d(xr, wr, None, padding=K // 2, groups=C)
    yref.backward(dyr)
    # (rnd returns fp32 tensors as they are, so x and w carry requires_grad from here on: detach what goes to the GPU)
    xg, dyg, taps = cl(x.detach(), dtype, dev), cl(dy, dtype, dev), _taps(w.detach(), dtype, dev)
    y = hip.dwconv3d(xg, taps, torch.empty_like(xg), K)
    check(ncdhw(y), yref.detach(), dtype, f"dwconv k{K} fwd")
    dx = hip.dwconv3d(dyg, taps, torch.empty_like(xg), K, flip=True)
    check(ncdhw(dx), xr.grad, dtype, f"dwconv k{K} input gradient")
    dw = torch.empty(C, 1, K, K, K, dtype=torch.float32, device=dev)
    hip.dwconv3d_wgrad(xg, dyg, dw, K)
    check(dw, wr.grad, dtype, f"dwconv k{K} wgrad")
    # two runs: same bits
    assert torch.equal(hip.dwconv3d(xg, taps, torch.empty_like(xg), K), y)
    assert torch.equal(hip.dwconv3d(dyg, taps, torch.empty_like(xg), K, flip=True), dx)
    dw2 = torch.empty_like(dw)
    hip.dwconv3d_wgrad(xg, dyg, dw2, K)
    assert torch.equal(dw2, dw)
    # accumulate: exactly twice
    hip.dwconv3d_wgrad(xg, dyg, dw2, K, True)
    assert torch.equal(dw2, dw + dw)
    # the input read from (and the result written into) a channel slice of a wider buffer: same bits, the rest untouched
    wide = torch.full((N,) + sp + (2 * C + 8,), 7.0, dtype=dtype, device=dev)
    wide[..., C:2 * C] = xg
    xs = wide[..., C:2 * C]
    assert hip.ld(xs) == 2 * C + 8
    assert torch.equal(hip.dwconv3d(xs, taps, torch.empty_like(xg), K), y)
    dw3 = torch.empty_like(dw)
    hip.dwconv3d_wgrad(xs, dyg, dw3, K)
    assert torch.equal(dw3, dw)
    out = torch.full((N,) + sp + (2 * C + 8,), 5.0, dtype=dtype, device=dev)
    hip.dwconv3d(xs, taps, out[..., :C], K)
    assert torch.equal(out[..., :C], y) and bool((out[..., C:] == 5.0).all())
    assert torch.equal(wide[..., C:2 * C], xg) and bool((wide[..., :C] == 7.0).all()) and bool((wide[..., 2 * C:] == 7.0).all())
    # the autograd function
    wp = torch.nn.Parameter(w.detach().to(dev))
    xa = xg.clone().requires_grad_(True)
    ya = ops.dwconv(xa, wp)
    assert torch.equal(ya.detach(), y)
    ya.backward(dyg)
    assert torch.equal(xa.grad, dx) and torch.equal(wp.grad, dw)
    if K == 3:
        y3 = ops.dwconv3(xg, wp.detach(), torch.zeros(C, device=dev))
        check(ncdhw(y3), yref.detach(), dtype, "dwconv3 (k3 kernel) fwd")
        check(y, y3, dtype, "dwconv k3 vs the k3 kernel")


def test_dwconv_large_refuses_unsupported():
    from medicalsemseg_amd import hip
    dev = torch.device(DEV)
    x = torch.zeros(1, 4, 4, 4, 8, device=dev)
    for K in (1, 4, 13):
        with pytest.raises(hip.MssegError):
            hip.dwconv3d(x, torch.zeros(K ** 3, 8, device=dev), torch.empty_like(x), K)
    x4 = torch.zeros(1, 4, 4, 4, 4, device=dev)          # a multiple of the fp32 chunk, not of 8
    with pytest.raises(hip.MssegError):
        hip.dwconv3d(x4, torch.zeros(27, 4, device=dev), torch.empty_like(x4), 3)
    with pytest.raises(hip.MssegError):
        hip.dwconv3d_wgrad(x4, x4, torch.zeros(4, 1, 3, 3, 3, device=dev), 3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,C,sp", [(9, 16, (8, 8, 8)), (11, 8, (6, 6, 6))])
def test_dwconv_large_integer_exact(dtype, K, C, sp):
    """integer-valued x in [-4, 4], w in [-2, 2], dy in [-2, 2]: every partial sum is an integer below 2^24 (at most
    11^3 * 8 = 10648 forward, 2 * 512 * 8 = 8192 in the weight gradient), so fp32 accumulation is exact in any order: forward
    and input gradient equal the CPU result rounded to the dtype bit for bit, the fp32 weight gradient equals it exactly"""
    from medicalsemseg_amd import hip
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(7)
    N = 2
    x = torch.randint(-4, 5, (N, C) + sp, generator=g).float()
    w = torch.randint(-2, 3, (C, 1, K, K, K), generator=g).float()
    dy = torch.randint(-2, 3, (N, C) + sp, generator=g).float()
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    yref = F.conv3d(xr.double(), wr.double(), None, padding=K // 2, groups=C)
    yref.backward(dy.double())
    xg, dyg, taps = cl(x, dtype, dev), cl(dy, dtype, dev), _taps(w, dtype, dev)
    y = hip.dwconv3d(xg, taps, torch.empty_like(xg), K)
    assert torch.equal(ncdhw(y), yref.detach().float().to(dtype).float())
    dx = hip.dwconv3d(dyg, taps, torch.empty_like(xg), K, flip=True)
    assert torch.equal(ncdhw(dx), xr.grad.float().to(dtype).float())
    dw = torch.empty(C, 1, K, K, K, dtype=torch.float32, device=dev)
    hip.dwconv3d_wgrad(xg, dyg, dw, K)
    assert torch.equal(dw.cpu(), wr.grad.float())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,sp", [(16, (4, 5, 6)), (48, (6, 6, 6))])
def test_focal_kernels(dtype, C, sp):
    """spatial mean, aggregate (forward / backward) and the modulation product, q and the gates read from (gradients written
    into) channel ranges of a [.., 2C + 8] buffer, against autograd of the same expressions in plain torch"""
    from medicalsemseg_amd import hip
    dev = torch.device(DEV)
    N, Fw = 2, 2 * C + 8
    S = sp[0] * sp[1] * sp[2]
    f, c1, c2, hm, da, dy = (rnd(dtype, gen(N, *sp, ch, seed=s)) for s, ch in ((1, Fw), (2, C), (3, C), (4, C), (5, C), (6, C)))
    fr, c1r, c2r, hr = (t.clone().requires_grad_(True) for t in (f, c1, c2, hm))
    q, gates = fr[..., :C], fr[..., 2 * C:2 * C + 3]
    mean = c2r.mean((1, 2, 3), keepdim=True)
    agg = c1r * gates[..., 0:1] + c2r * gates[..., 1:2] + F.gelu(mean) * gates[..., 2:3]
    prod = q * hr
    ((agg * da).sum() + (prod * dy).sum()).backward()
    fg, c1g, c2g, hg, dag, dyg = (t.to(dev, dtype) for t in (f, c1, c2, hm, da, dy))
    gv = fg[..., 2 * C:]
    m = torch.empty(N, C, dtype=torch.float32, device=dev)
    gm = torch.empty_like(m)
    hip.focal_spatial_sum(c2g, m, gm, scale=1.0 / S, mode=0)
    check(m, mean.detach().reshape(N, C), dtype, "spatial mean")
    check(gm, F.gelu(mean.detach()).reshape(N, C), dtype, "GELU of the mean")
    m2, gm2 = torch.empty_like(m), torch.empty_like(m)
    hip.focal_spatial_sum(c2g, m2, gm2, scale=1.0 / S, mode=0)
    assert torch.equal(m2, m) and torch.equal(gm2, gm)
    out = hip.focal_aggregate_fwd(c1g, c2g, gv, gm, torch.empty_like(c1g))
    check(out, agg.detach(), dtype, "aggregate fwd")
    df = torch.full_like(fg, 3.0)
    dmv = torch.empty_like(m)
    hip.focal_spatial_sum(dag, dmv, None, g=gv[..., 2:3], m_in=m, scale=1.0 / S, mode=1)
    dc1, dc2 = torch.empty_like(c1g), torch.empty_like(c2g)
    hip.focal_aggregate_bwd(dag, c1g, c2g, gv, gm, dmv, dc1, dc2, df[..., 2 * C:])
    check(dc1, c1r.grad, dtype, "aggregate bwd: first context")
    check(dc2, c2r.grad, dtype, "aggregate bwd: second context (with the mean's gradient)")
    check(df[..., 2 * C:2 * C + 3], fr.grad[..., 2 * C:2 * C + 3], dtype, "aggregate bwd: gates")
    assert bool((df[..., 2 * C + 3:] == 0).all()) and bool((df[..., :2 * C] == 3.0).all())
    y = hip.focal_mul_fwd(fg[..., :C], hg, torch.empty_like(hg))
    check(y, prod.detach(), dtype, "product fwd")
    dh = torch.empty_like(hg)
    hip.focal_mul_bwd(dyg, fg[..., :C], hg, df[..., :C], dh)
    check(df[..., :C], fr.grad[..., :C], dtype, "product bwd: q")
    check(dh, hr.grad, dtype, "product bwd: h")
    assert bool((df[..., C:2 * C] == 3.0).all())


def _rel(a, b):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else a
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def test_focalnet_encoder_vs_reference_golden(golden_dir):
    """HIP encoder (fp32 compute) against vectors of the REFERENCE's own FocalNet (tools/gen_golden_focalnet.py); gates of
    test_swin_encoder_vs_reference_golden"""
    from medicalsemseg_amd.models.focalnet import FocalNet
    from tests.focalnet_ref import FocalNetRef
    g = np.load(os.path.join(golden_dir, "focalnet_encoder_v32.npz"))
    vol = (32, 32, 32)
    src = FocalNetRef(vol, **GOLD_CFG)       # reference-shaped parameters carry the deterministic fill
    det_fill_(src, "focal")
    m = FocalNet(vol, drop_path_rate=0.0, compute_dtype=torch.float32, **GOLD_CFG)
    m.load_state_dict(src.state_dict(), strict=True)
    m = m.to(DEV)
    x = det_tensor("focal_x", (2, 1) + vol).to(DEV)
    feats, _ = m((x, None, None))
    assert len(feats) == 4
    loss = 0
    for i, f in enumerate(feats):
        ref = g[f"out{i}"]
        got = f.permute(0, 4, 1, 2, 3)
        print(f"feature {i}: {_rel(got, ref):.3e}")
        assert _rel(got, ref) < 1e-3, f"feature {i}"
        loss = loss + (got * det_tensor(f"focal_r{i}", ref.shape).to(DEV)).sum()
    loss.backward()
    mod0, mod1 = m.layers[0].blocks[0].modulation, m.layers[1].blocks[0].modulation
    assert _rel(mod0.focal_layers[1][0].weight.grad, g["d_focal_k5"]) < 5e-3
    assert _rel(mod0.f.weight.grad[:35], g["d_f_w"]) < 5e-3
    assert bool((mod0.f.weight.grad[35:] == 0).all()) and bool((mod0.f.bias.grad[35:] == 0).all())
    assert _rel(mod0.h.weight.grad, g["d_h_w"]) < 5e-3
    assert _rel(mod1.focal_layers[1][0].weight.grad, g["d_focal_k7"]) < 5e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_focalnet_unetr_vs_oracle(dtype):
    """whole FocalNetUNETR (64^3, width 16, depths 1-1-1-1, windows 3-5-3-3, 3 classes, batch 2): forward + DiceCE + backward
    against tests/focalnet_ref.py inside oracle.swin.SwinUNETRCustom; written and gated like
    tests/test_gpu_swin.py::test_swin_unetr_vs_oracle.  64^3 is the smallest volume four stages at patch 2 take: at 32^3 the
    deepest feature map is 1^3 and the decoder's InstanceNorm (torch's, in the oracle) refuses a single spatial element.
    Token grids 32-16-8-4, deepest map 2^3."""
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models import swin_unetr as P
    from medicalsemseg_amd.models.focalnet import FocalNet
    from oracle import swin as O
    from oracle.losses import dice_ce_loss
    from tests.focalnet_ref import FocalNetRef
    from tests.test_gpu_swin import BF16_GATES
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    vol, hs = (64, 64, 64), 16
    kw = dict(patch_size=(2, 2, 2), in_chans=1, embed_dim=hs, depths=(1, 1, 1, 1), focal_windows=(3, 5, 3, 3))
    ref = O.SwinUNETRCustom(FocalNetRef(vol, **kw), 1, 3, hs, 2)
    enc = FocalNet(vol, drop_path_rate=0.0, compute_dtype=dtype, **kw)
    net = P.SwinUNETRCustom(enc, 1, 3, vol, hs, (2, 2, 2), compute_dtype=dtype)
    net.load_state_dict(dict(ref.state_dict()), strict=True)
    net = net.to(DEV)
    x = det_tensor("focal_su_x", (2, 1) + vol)
    gl = torch.Generator().manual_seed(3)
    y = torch.randint(0, 3, (2, 1) + vol, generator=gl).float()
    out_ref = ref((x, None, None))
    loss_ref = dice_ce_loss(out_ref, y)
    loss_ref.backward()
    out = net((x.to(DEV), None, None))
    loss = DiceCELoss()(out, y.to(DEV))
    loss.backward()
    dl = abs(float(loss.detach()) - float(loss_ref.detach()))
    print(f"[{dtype}] FocalNetUNETR 64^3: logits err/scale {_rel(out, out_ref.detach().numpy()):.3e}, |loss diff| {dl:.2e}")
    if dtype == torch.float32:
        np.testing.assert_allclose(out.detach().cpu().numpy(), out_ref.detach().numpy(), rtol=1e-4, atol=2e-4)
        assert dl < 1e-4
    else:
        assert _rel(out, out_ref.detach().numpy()) < BF16_GATES["swin32"][0]
        assert dl < BF16_GATES["swin32"][1]
    pr = dict(ref.named_parameters())
    num = den = 0.0
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        gr = pr[name].grad
        got = p.grad.cpu()
        if got.shape != gr.shape:                      # modulation.f: zero-padded rows
            pad = got[gr.shape[0]:]
            assert bool((pad == 0).all()), name
            got = got[:gr.shape[0]]
        num += float(((got - gr) ** 2).sum())
        den += float((gr ** 2).sum())
    tot = (num / den) ** 0.5
    print(f"[{dtype}] FocalNetUNETR 64^3 whole-net grad rel-L2 {tot:.3e}")
    assert tot < (2e-3 if dtype == torch.float32 else BF16_GATES["swin32"][2]), f"whole-net grad rel L2 err {tot:.3e}"
    with torch.no_grad():
        out2 = net((x.to(DEV), None, None))
    assert torch.equal(out2, out.detach())


def test_focalnet_unetr_train_steps():
    """three FlatAdamW steps (bf16, 64^3, width 16, stochastic depth 0.2 with fixed masks) on synthetic blobs: the loss is
    finite and falls, a repeated run gives the same bits, the padded rows of every modulation.f stay exactly zero and the
    state dict loads back strictly"""
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models import swin_unetr as P
    from medicalsemseg_amd.models.focalnet import FocalNet, _FocalBlock, _FocalF
    from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay
    vol, hs = (64, 64, 64), 16
    kw = dict(patch_size=(2, 2, 2), in_chans=1, embed_dim=hs, depths=(2, 1, 1, 1), focal_windows=(5, 3, 3, 3))
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 1, *vol, generator=g).to(DEV)
    y = _blobs(2, 64, 3, 14).to(DEV)
    crit = DiceCELoss()

    def make():
        torch.manual_seed(0)
        enc = FocalNet(vol, drop_path_rate=0.2, compute_dtype=torch.bfloat16, **kw)
        n = P.SwinUNETRCustom(enc, 1, 3, vol, hs, (2, 2, 2), compute_dtype=torch.bfloat16).to(DEV)
        n.train()
        blocks = [m for m in n.modules() if isinstance(m, _FocalBlock)]
        assert blocks[-1].drop_path == pytest.approx(0.2) and blocks[0].drop_path == 0.0
        for i, b in enumerate(blocks):               # one sample dropped in every other block
            b.dp_mask = torch.tensor([1.0, float(i % 2 == 0)])
        return n, FlatAdamW(add_weight_decay(n, 1e-5), lr=4e-4, betas=(0.9, 0.95), eps=1e-6)

    def run():
        n, opt = make()
        losses = []
        for _ in range(3):
            loss = crit(n((x, None, None)), y)
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(float(loss))
        return n, losses, opt.flat_param.clone()

    na, la, pa = run()
    _, lb, pb = run()
    print("FocalNetUNETR training losses", la)
    assert all(np.isfinite(la)) and la[-1] < la[0]
    assert la == lb and torch.equal(pa, pb)
    fs = [m for m in na.modules() if isinstance(m, _FocalF)]
    assert len(fs) == 5
    for m in fs:
        real = m._real["bias"][0]
        assert bool((m.weight[real:] == 0).all()) and bool((m.bias[real:] == 0).all())
        assert float(m.weight[:real].abs().max()) > 0
    sd = na.state_dict()
    assert tuple(sd["encoder.layers.0.blocks.0.modulation.f.weight"].shape) == (2 * hs + 3, hs)
    nb, _ = make()
    nb.load_state_dict(sd, strict=True)
    for (name, p), (_, q) in zip(na.named_parameters(), nb.named_parameters()):
        assert torch.equal(p, q), name
