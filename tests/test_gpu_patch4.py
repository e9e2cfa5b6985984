"""GPU parity of patch size 4 (the nnFormer setting): ConvTranspose3d k = s = 4 and the k = 4 patch embedding against
stock torch-CPU fp32 ops (the tolerance rule of tests/test_gpu_kernels.py), the HIP encoder against the fixture the
REFERENCE's own encoder produced at patch size 4, the whole patch-4 Swin-UNETR against the CPU oracle, and training steps."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.golden_util import det_fill_, det_tensor
from tests.test_gpu_baseline import _blobs, _grad_rel_l2, _soft_dice_term
from tests.test_gpu_kernels import DTYPES, check, cl, gen, ncdhw, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,sp", [(48, 48, (6, 6, 6)), (32, 32, (3, 5, 19)),     # ragged W: a last group of 3 voxels
                                         (96, 96, (2, 3, 17)), (64, 64, (4, 4, 4)),
                                         (48, 48, (24, 24, 24)),                        # the production shape (96^3, batch 2)
                                         (16, 16, (3, 4, 5)), (24, 24, (3, 4, 5))])     # off the bf16 fast path
def test_deconv_k4s4(dtype, cin, cout, sp):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.layers import Deconv2
    dev = torch.device(DEV)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    N = 2
    x = gen(N, cin, *sp, seed=1)
    w = gen(cin, cout, 4, 4, 4, seed=2, scale=cin ** -0.5)
    b = gen(cout, seed=3)
    xr, wr = rnd(dtype, x, w)
    xr.requires_grad_(True); wr.requires_grad_(True)
    yref = F.conv_transpose3d(xr, wr, b, stride=4)
    dy = gen(*yref.shape, seed=4)
    dyr = rnd(dtype, dy)
    yref.backward(dyr)
    wp = torch.nn.Parameter(w.to(dev)); bp = torch.nn.Parameter(b.to(dev))
    op = Deconv2(wp, bp)
    assert op.k == 4
    xg = cl(x, dtype, dev)
    y = op.fwd(xg)
    assert tuple(y.shape) == (N, 4 * sp[0], 4 * sp[1], 4 * sp[2], cout)
    check(ncdhw(y), yref.detach(), dtype, "deconv4 fwd")
    # into the first cout channels of a wider (concat) buffer: same bits, the other channels untouched
    cat = torch.full((N, 4 * sp[0], 4 * sp[1], 4 * sp[2], 2 * cout), 7.0, dtype=dtype, device=dev)
    op.fwd(xg, out=cat[..., :cout])
    assert torch.equal(cat[..., :cout], y) and bool((cat[..., cout:] == 7.0).all())
    assert torch.equal(op.fwd(xg), y)                                     # two runs: same bits
    del yref
    # backward, the gradient read from a channel slice of a wider buffer as UpBlock hands it over
    dcat = torch.zeros(N, 4 * sp[0], 4 * sp[1], 4 * sp[2], 2 * cout, dtype=dtype, device=dev)
    dcat[..., :cout] = cl(dy, dtype, dev)
    dyg = dcat[..., :cout]
    dx = op.bwd(xg, dyg, True)
    torch.cuda.synchronize()
    check(ncdhw(dx), xr.grad, dtype, "deconv4 bwd data")
    check(wp.grad, wr.grad, dtype, "deconv4 wgrad")
    check(bp.grad, dyr.sum((0, 2, 3, 4)), dtype, "deconv4 bias grad")
    # dense gradient: same bits as from the slice; accumulate-twice; two runs of each kernel bit-identical
    dyd = dyg.contiguous()
    wpd = hip.pack_deconv(wp.detach(), dtype, bwd=True)
    dx2 = torch.empty_like(dx)
    hip.deconv_k4s4_bwd_data(dyd, wpd, dx2, cin, cout)
    assert torch.equal(dx2, dx)
    dw = torch.empty_like(wp)
    hip.deconv_k4s4_wgrad(xg, dyd, dw, cin, cout)
    assert torch.equal(dw, wp.grad)
    dw1 = dw.clone()
    hip.deconv_k4s4_wgrad(xg, dyd, dw, cin, cout, True)
    check(dw, 2 * wr.grad, dtype, "deconv4 wgrad accumulate")
    assert torch.equal(dw, dw1 + dw1)
    dw3 = torch.empty_like(wp)
    hip.deconv_k4s4_wgrad(xg, dyg, dw3, cin, cout)
    assert torch.equal(dw3, dw1)
    # without the input gradient: weight and bias gradients only (accumulating onto the first pass)
    assert op.bwd(xg, dyg, False) is None
    torch.cuda.synchronize()
    check(wp.grad, 2 * wr.grad, dtype, "deconv4 wgrad second pass")
    check(bp.grad, 2 * dyr.sum((0, 2, 3, 4)), dtype, "deconv4 bias grad second pass")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin", [1, 2])
def test_patch_embed_k4(dtype, cin):
    """PatchEmbed3D.proj at patch size 4: Conv3d k = s = 4 on the few-channel gather kernels (K = cin * 64 <= 128)"""
    from medicalsemseg_amd import ops
    dev = torch.device(DEV)
    cout, sp = 48, (12, 16, 20)
    x = gen(2, cin, *sp, seed=1)
    w = gen(cout, cin, 4, 4, 4, seed=2, scale=(cin * 64) ** -0.5)
    b = gen(cout, seed=3)
    xr, wr = rnd(dtype, x, w)
    wr.requires_grad_(True)
    br = b.clone().requires_grad_(True)
    yref = F.conv3d(xr, wr, br, stride=4)
    dy = gen(*yref.shape, seed=4)
    dyr = rnd(dtype, dy)
    yref.backward(dyr)
    wp = torch.nn.Parameter(w.to(dev)); bp = torch.nn.Parameter(b.to(dev))
    y = ops.PatchConvFn.apply(cl(x, dtype, dev), wp, bp, 4)
    assert tuple(y.shape) == (2, 3, 4, 5, cout)
    check(ncdhw(y.detach()), yref.detach(), dtype, "patch embed k4 fwd")
    y.backward(cl(dy, dtype, dev))
    check(wp.grad, wr.grad, dtype, "patch embed k4 wgrad")
    check(bp.grad, br.grad, dtype, "patch embed k4 bias grad")


@pytest.mark.parametrize("cin,cout,sp", [(48, 48, (3, 5, 19)), (64, 32, (6, 7, 9))])
def test_deconv_k2s2_unchanged(cin, cout, sp):
    """the layer class generalised over k gives, for k = 2 weights, the bits of the direct k2 s2 entry points"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.layers import Deconv2
    dev = torch.device(DEV)
    dtype = torch.bfloat16
    x = cl(gen(2, cin, *sp, seed=1), dtype, dev)
    wp = torch.nn.Parameter(gen(cin, cout, 2, 2, 2, seed=2, scale=cin ** -0.5).to(dev))
    dy = cl(gen(2, cout, 2 * sp[0], 2 * sp[1], 2 * sp[2], seed=4), dtype, dev)
    op = Deconv2(wp, None)
    assert op.k == 2
    y = op.fwd(x)
    dx = op.bwd(x, dy, True)
    torch.cuda.synchronize()
    y2 = torch.empty_like(y)
    hip.deconv_k2s2(x, hip.pack_deconv(wp.detach(), dtype), None, y2, cin, cout)
    dx2 = torch.empty_like(dx)
    hip.deconv_k2s2_bwd_data(dy, hip.pack_deconv(wp.detach(), dtype, bwd=True), dx2, cin, cout)
    dw2 = torch.empty_like(wp)
    hip.deconv_k2s2_wgrad(x, dy, dw2, cin, cout)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(wp.grad, dw2)


def _rel(a, b):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else a
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def test_swin_encoder_p4_vs_reference_golden(golden_dir):
    """HIP encoder (fp32 compute) at patch size 4 against vectors of the REFERENCE's own SwinTransformerNNFormer
    (tools/gen_golden_patch4.py); gates of test_swin_encoder_vs_reference_golden"""
    from medicalsemseg_amd.models.swin_unetr import SwinTransformerNNFormer
    g = np.load(os.path.join(golden_dir, "swin_encoder_p4_v48.npz"))
    vol = (48, 48, 48)
    m = SwinTransformerNNFormer(vol, (4, 4, 4), 1, 32, (2, 2), (2, 4), (6, 3), drop_path_rate=0.0, compute_dtype=torch.float32)
    det_fill_(m, "enc_p4")
    m = m.to(DEV)
    x = det_tensor("enc_p4_x", (2, 1) + vol).to(DEV)
    feats, _ = m((x, None, None))
    assert len(feats) == 3
    loss = 0
    for i, f in enumerate(feats):
        ref = g[f"out{i}"]
        got = f.permute(0, 4, 1, 2, 3)
        assert _rel(got, ref) < 1e-3, f"feature {i}"
        loss = loss + (got * det_tensor(f"enc_p4_r{i}", ref.shape).to(DEV)).sum()
    loss.backward()
    assert _rel(m.layers[0].blocks[1].attn.qkv.weight.grad, g["d_qkv_w"]) < 5e-3
    assert _rel(m.patch_embed.proj.weight.grad, g["d_proj_w"]) < 5e-3
    assert _rel(m.patch_embed.proj.bias.grad, g["d_proj_b"]) < 5e-3


# bf16 gates of the 96^3 hidden-48 patch-4 net vs the fp32 CPU oracle (logits err / scale, whole-net gradient rel-L2,
# |loss difference|): twice the values measured on MI355X -- logits 7.37e-3, gradients 2.30e-3, |loss diff| 8.43e-4, soft Dice
# 1.3e-4 -- never above the patch-2 gates of tests/test_gpu_baseline.py::test_swin_unetr_48_config_vs_oracle
# (1.8e-2 / 6e-3 / 1e-3).  The loss gate sits AT that cap (twice the measured value would be 1.7e-3): the bf16 loss drift of
# the patch-4 net is about twice the patch-2 net's (3.9e-4), with 18 % headroom under the gate.
P4_BF16_GATES = (1.5e-2, 4.6e-3, 1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swin_unetr_p4_vs_oracle(dtype):
    """hidden 48, patch 4, 96^3, depths 2-2-2, heads 3-6-12, windows 6-6-3, one sample: logits, DiceCE loss and all
    parameter gradients against oracle.swin (pyramid 24-12-6-3; the last up block is the k4 s4 transposed conv)"""
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models import swin_unetr as P
    from oracle import swin as O
    from oracle.losses import dice_ce_loss
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    vol, hs = (96, 96, 96), 48
    kw = dict(patch_size=(4, 4, 4), in_chans=1, embed_dim=hs, depths=(2, 2, 2), num_heads=(3, 6, 12), window_size=(6, 6, 3))
    ref = O.SwinUNETRCustom(O.SwinTransformerNNFormer(vol, **kw), 1, 3, hs, 4)
    enc = P.SwinTransformerNNFormer(vol, drop_path_rate=0.0, compute_dtype=dtype, **kw)
    net = P.SwinUNETRCustom(enc, 1, 3, vol, hs, (4, 4, 4), compute_dtype=dtype)
    net.load_state_dict(dict(ref.state_dict()), strict=True)
    net = net.to(DEV)
    x = det_tensor("su48p4_x", (1, 1) + vol)
    y = _blobs(1, 96, 3, 3)
    out_ref = ref((x, None, None))
    loss_ref = dice_ce_loss(out_ref, y)
    loss_ref.backward()
    out = net((x.to(DEV), None, None))
    assert tuple(out.shape) == (1, 3, 96, 96, 96)
    loss = DiceCELoss()(out, y.to(DEV))
    loss.backward()
    o = out.detach().float().cpu()
    tot, worst = _grad_rel_l2(net, ref, skip_bias_before_norm=False)
    scale = float(out_ref.detach().abs().max())
    err = float((o - out_ref.detach()).abs().max()) / scale
    dl = abs(float(loss) - float(loss_ref))
    print(f"[{dtype}] Swin-UNETR-48 patch 4 96^3: logits err/scale {err:.3e}, loss {float(loss):.5f} vs {float(loss_ref):.5f} "
          f"(|diff| {dl:.2e}), grad rel-L2 {tot:.3e}, worst {worst}")
    if dtype == torch.float32:
        np.testing.assert_allclose(o.numpy(), out_ref.detach().numpy(), rtol=1e-4, atol=2e-4 * max(scale, 1.0))
        assert dl < 1e-4
        assert tot < 2e-3
    sd, sd_ref = _soft_dice_term(o, y), _soft_dice_term(out_ref.detach(), y)
    print(f"[{dtype}] Swin-UNETR-48 patch 4 96^3 soft-Dice term {sd:.6f} vs oracle {sd_ref:.6f}")
    assert abs(sd - sd_ref) < 1e-3
    if dtype == torch.bfloat16:
        assert err < P4_BF16_GATES[0] and tot < P4_BF16_GATES[1] and dl < P4_BF16_GATES[2]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swin_unetr_p4_small_vs_oracle(dtype):
    """64^3, hidden 16 (the plain vector kernels of the k4 s4 transposed conv), depths 2-2-2, heads 1-2-4, windows 4-4-4,
    batch 2; written and gated like tests/test_gpu_swin.py::test_swin_unetr_vs_oracle"""
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models import swin_unetr as P
    from oracle import swin as O
    from oracle.losses import dice_ce_loss
    from tests.test_gpu_swin import BF16_GATES
    torch.manual_seed(0)
    vol, hs = (64, 64, 64), 16
    kw = dict(patch_size=(4, 4, 4), in_chans=1, embed_dim=hs, depths=(2, 2, 2), num_heads=(1, 2, 4), window_size=(4, 4, 4))
    ref = O.SwinUNETRCustom(O.SwinTransformerNNFormer(vol, **kw), 1, 3, hs, 4)
    enc = P.SwinTransformerNNFormer(vol, drop_path_rate=0.0, compute_dtype=dtype, **kw)
    net = P.SwinUNETRCustom(enc, 1, 3, vol, hs, (4, 4, 4), compute_dtype=dtype)
    net.load_state_dict(dict(ref.state_dict()), strict=True)
    net = net.to(DEV)
    x = det_tensor("sup4_x", (2, 1) + vol)
    gl = torch.Generator().manual_seed(3)
    y = torch.randint(0, 3, (2, 1) + vol, generator=gl).float()
    out_ref = ref((x, None, None))
    loss_ref = dice_ce_loss(out_ref, y)
    loss_ref.backward()
    out = net((x.to(DEV), None, None))
    loss = DiceCELoss()(out, y.to(DEV))
    loss.backward()
    dl = abs(float(loss.detach()) - float(loss_ref.detach()))
    print(f"[{dtype}] Swin-UNETR patch 4 64^3: logits err/scale {_rel(out, out_ref.detach().numpy()):.3e}, |loss diff| {dl:.2e}")
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
        num += float(((p.grad.cpu() - gr) ** 2).sum())
        den += float((gr ** 2).sum())
    tot = (num / den) ** 0.5
    print(f"[{dtype}] Swin-UNETR patch 4 64^3 whole-net grad rel-L2 {tot:.3e}")
    assert tot < (2e-3 if dtype == torch.float32 else BF16_GATES["swin32"][2]), f"whole-net grad rel L2 err {tot:.3e}"
    # inference under no_grad goes through the same forward
    with torch.no_grad():
        out2 = net((x.to(DEV), None, None))
    assert torch.equal(out2, out.detach())


def test_swin_unetr_p4_train_steps():
    """three FlatAdamW steps on a patch-4 model (bf16, 64^3, hidden 32, two stages): the loss is finite and falls, the run
    repeated gives the same bits, and the two-phase backward gives the single-phase gradients bit for bit"""
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models import swin_unetr as P
    from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay
    vol, hs = (64, 64, 64), 32
    kw = dict(patch_size=(4, 4, 4), in_chans=1, embed_dim=hs, depths=(2, 2), num_heads=(2, 4), window_size=(4, 4))
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 1, *vol, generator=g).to(DEV)
    y = _blobs(2, 64, 3, 14).to(DEV)
    crit = DiceCELoss()

    def make():
        torch.manual_seed(0)
        enc = P.SwinTransformerNNFormer(vol, drop_path_rate=0.0, compute_dtype=torch.bfloat16, **kw)
        n = P.SwinUNETRCustom(enc, 1, 3, vol, hs, (4, 4, 4), compute_dtype=torch.bfloat16).to(DEV)
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
        return losses, opt.flat_param.clone()

    la, pa = run()
    lb, pb = run()
    print("patch-4 training losses", la)
    assert all(np.isfinite(la)) and la[-1] < la[0]
    assert la == lb and torch.equal(pa, pb)

    net, opt = make()
    crit(net((x, None, None)), y).backward()
    ref = opt.flat_grad.clone()
    opt.zero_grad()
    net.defer_backward_tail(True)
    crit(net((x, None, None)), y).backward()
    net.backward_tail()
    assert torch.equal(opt.flat_grad, ref)
    net.defer_backward_tail(False)
