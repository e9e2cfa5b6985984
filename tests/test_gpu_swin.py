"""GPU parity of the Swin path: HIP window attention / Swin block / encoder against the golden vectors produced by
the REFERENCE's own modules (tests/golden, oracle/gen_golden.py), and the whole Swin-UNETR against the oracle."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

from tests.golden_util import det_fill_, det_tensor

pytestmark = pytest.mark.gpu

# bf16 whole-net gates (logits err / scale, |loss difference|, whole-net gradient rel-L2) vs the fp32 CPU oracle: about twice
# the values measured on MI355X (printed by the tests), so that a 2-3x regression of the bf16 path fails
BF16_GATES = {"swin32": (1.6e-2, 1e-3, 4.5e-2),      # measured 7.8e-3, 7e-6, 2.1e-2
              "official64": (2e-2, 5e-3, 4e-2)}      # measured 1.03e-2, -, 1.9e-2
DEV = "cuda:0"


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _rel(a, b):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else a
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _windows_to_volume(xw, ws, shift):
    """[8, N, C] windows of the SHIFTED (2ws)^3 grid -> unshifted volume [1, 2ws, 2ws, 2ws, C]"""
    from oracle.swin import window_reverse
    C = xw.shape[-1]
    vol = window_reverse(xw.reshape(8, ws, ws, ws, C), ws, 2 * ws, 2 * ws, 2 * ws)
    return torch.roll(vol, shifts=(shift, shift, shift), dims=(1, 2, 3))


def _volume_to_windows(vol, ws, shift):
    from oracle.swin import window_partition
    v = torch.roll(vol, shifts=(-shift, -shift, -shift), dims=(1, 2, 3))
    return window_partition(v, ws).reshape(8, ws ** 3, -1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tag,dim,ws,heads", [("h3w6", 48, 6, 3), ("h24w3", 384, 3, 24)])
def test_window_attention_vs_reference_golden(golden_dir, dtype, tag, dim, ws, heads):
    from medicalsemseg_amd import ops
    from medicalsemseg_amd.models.swin_unetr import _WindowAttention
    g = _load(golden_dir, f"swin_attn_{tag}.npz")
    m = _WindowAttention(dim, ws, heads, True)
    det_fill_(m, "attn_" + tag)
    m = m.to(DEV)
    N = ws ** 3
    xw = det_tensor("attn_x_" + tag, (8, N, dim))
    rw = det_tensor("attn_r_" + tag, (8, N, dim))
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    for mk, shift in (("nomask", 0), ("mask", ws // 2)):
        x = _windows_to_volume(xw, ws, shift).to(DEV, dtype).requires_grad_(True)
        r = _windows_to_volume(rw, ws, shift).to(DEV, dtype)
        for p in m.parameters():
            p.grad = None
        qkv = ops.linear(x, m.qkv.weight, m.qkv.bias)
        y = ops.WindowAttnFn.apply(qkv, m.qkv.bias, m.relative_position_bias_table, heads, ws, shift)
        y = ops.linear(y, m.proj.weight, m.proj.bias)
        (y.float() * r.float()).sum().backward()
        assert _rel(_volume_to_windows(y.detach().float().cpu(), ws, shift), g[f"y_{mk}"]) < tol
        assert _rel(_volume_to_windows(x.grad.float().cpu(), ws, shift), g[f"dx_{mk}"]) < tol
        assert _rel(m.relative_position_bias_table.grad, g[f"dtable_{mk}"]) < (1e-3 if dtype == torch.float32 else 5e-2)
        if f"dqkvw_{mk}" in g.files:
            assert _rel(m.qkv.weight.grad, g[f"dqkvw_{mk}"]) < (1e-3 if dtype == torch.float32 else 5e-2)


@pytest.mark.parametrize("R,ws,heads,C,shift", [(12, 6, 3, 48, 0), (10, 6, 3, 48, 3), (6, 3, 4, 64, 1)])
def test_attention_bwd_table_gradient_workspace_path_equals_atomics_path(monkeypatch, R, ws, heads, C, shift):
    """bf16 MFMA backward: the bias-table gradient from the dS workspace (window sum + gather, deterministic) against the
    LDS-atomics form of the same kernel; dqkv is the same arithmetic in both (R = 10 pads the volume to 12)."""
    from medicalsemseg_amd import hip
    torch.manual_seed(5)
    qkv = torch.randn(2, R, R, R, 3 * C, device=DEV).bfloat16()
    qb = torch.randn(3 * C, device=DEV)
    tab = torch.randn((2 * ws - 1) ** 3, heads, device=DEV) * 0.1
    out = torch.empty(2, R, R, R, C, device=DEV, dtype=torch.bfloat16)
    dout = torch.randn_like(out)
    lse = hip.window_attention_fwd(qkv, qb, tab, out, heads, ws, shift)
    res = []
    for no_ws in (False, True):
        if no_ws:
            monkeypatch.setenv("MSSEG_ATTN_BWD_NO_WS", "1")
        else:
            monkeypatch.delenv("MSSEG_ATTN_BWD_NO_WS", raising=False)
        dqkv = torch.empty_like(qkv)
        dtab = torch.full_like(tab, 0.5)          # accumulate semantics: += on both paths
        hip.window_attention_bwd(qkv, qb, tab, out, lse, dout, dqkv, dtab, heads, ws, shift)
        res.append((dqkv.float(), dtab.clone()))
    monkeypatch.delenv("MSSEG_ATTN_BWD_NO_WS", raising=False)
    assert torch.equal(res[0][0], res[1][0])
    d = (res[0][1] - res[1][1]).norm() / (res[1][1] - 0.5).norm()
    assert float(d) < 5e-3                        # dS rounded to bf16 before the sum over windows
    # deterministic: a second call gives the same bits
    dtab2 = torch.full_like(tab, 0.5)
    hip.window_attention_bwd(qkv, qb, tab, out, lse, dout, torch.empty_like(qkv), dtab2, heads, ws, shift)
    assert torch.equal(dtab2, res[0][1])


@pytest.mark.parametrize("shift", [0, 3])
def test_swin_block_vs_reference_golden(golden_dir, shift):
    from medicalsemseg_amd.models.swin_unetr import _Block
    g = _load(golden_dir, "swin_block.npz")
    m = _Block(48, (12, 12, 12), 3, 6, shift, 4.0, True, 0.0)
    det_fill_(m, "blk")
    m = m.to(DEV)
    x = det_tensor("blk_x", (2, 12 ** 3, 48)).reshape(2, 12, 12, 12, 48).to(DEV).requires_grad_(True)
    y = m(x)
    assert _rel(y.reshape(2, -1, 48), g[f"y_shift{shift}"]) < 2e-4
    if shift:
        r = det_tensor("blk_r", (2, 12 ** 3, 48)).reshape(2, 12, 12, 12, 48).to(DEV)
        (y * r).sum().backward()
        assert _rel(x.grad.reshape(2, -1, 48), g["dx_shift3"]) < 1e-3


BLOCK_AFF = [[1.5, 0.8, 2.0], [-0.7, 1.25, 3.0]]


@functools.lru_cache(maxsize=None)
def _block_ref(res, ws, shift, affine):
    """float64 CPU: oracle.swin.SwinTransformerBlock under the deterministic parameters of the product block; with the
    spacing-conditioned bias its attention core is tests.attention_ref (pinned to this very block by
    tests/test_attention_ref_host.py) under per-sample tables folded from table, emb and lin in float64.  One reference serves
    both dtypes: x and r hold bf16-exact values."""
    from medicalsemseg_amd.models.swin_unetr import _Block
    from oracle import swin as O
    from tests.attention_ref import window_attention_ref
    dim, heads = 48, 3
    m = _Block(dim, res, heads, ws, shift, 4.0, True, 0.0, rel_pos_bias_affine=affine)
    det_fill_(m, "blkpad")
    ref = O.SwinTransformerBlock(dim, res, heads, ws, shift).double()
    extra = ref.load_state_dict(m.state_dict(), strict=False)
    assert not extra.missing_keys and all("rel_pos_bias_affine" in k for k in extra.unexpected_keys)
    S, H, W = res
    x = det_tensor("blkpad_x", (2, S, H, W, dim)).bfloat16().double().requires_grad_(True)
    r = det_tensor("blkpad_r", (2, S, H, W, dim)).bfloat16().double()
    a = ref.attn
    params = dict(ref.named_parameters())
    if affine:
        emb = m.attn.rel_pos_bias_affine_emb.detach().double().requires_grad_(True)
        lw = m.attn.rel_pos_bias_affine_lin.weight.detach().double().requires_grad_(True)
        lb = m.attn.rel_pos_bias_affine_lin.bias.detach().double().requires_grad_(True)
        aff = torch.tensor(BLOCK_AFF, dtype=torch.float64)
        tabs = a.relative_position_bias_table[None] + lb + (emb[None] * (lw[0] * aff)[:, None, None, :]).sum(-1)
        params.update({"attn.rel_pos_bias_affine_emb": emb, "attn.rel_pos_bias_affine_lin.weight": lw,
                       "attn.rel_pos_bias_affine_lin.bias": lb})
        qkv = a.qkv(ref.norm1(x))
        out, _, _ = window_attention_ref(qkv, a.qkv.bias, tabs, heads, ws, shift)
        h = x + a.proj(out)
        y = h + ref.mlp(ref.norm2(h))
    else:
        full = [-(-v // ws) * ws for v in res]
        y = ref(x.reshape(2, -1, dim), O.shift_region_mask(*full, ws, shift).double()).reshape(2, S, H, W, dim)
    (y * r).sum().backward()
    return m, x.detach(), r, y.detach(), x.grad, {k: p.grad for k, p in params.items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("res,ws,shift", [((5, 8, 7), 3, 1), ((10, 10, 10), 6, 3)])
def test_swin_block_on_padded_grids_vs_float64_oracle(res, ws, shift, affine, dtype):
    """models.swin_unetr._Block on grids that are no window multiple (10^3 under window 6: 42 % of the windows' tokens are
    padding) against oracle.swin.SwinTransformerBlock in float64: y, dx and the gradient of EVERY parameter, attn.qkv.bias among
    them, whose gradient takes the share of the padded tokens (the reference pads before its qkv Linear: Linear(0) = bias).
    Gates of test_swin_official_encoder_vs_reference_golden for the same quantities in fp32 (features 1e-3, parameter
    gradients 5e-3; dx under the 1e-3 of test_swin_block_vs_reference_golden), of test_window_attention_vs_reference_golden in
    bf16 (3e-2, 5e-2).  lin.bias' gradient is a sum of all dS, zero up to rounding: gated against the L1 mass of the table
    gradient, as tests/test_gpu_affine_bias.py does."""
    m, x64, r64, y64, dx64, grads = _block_ref(res, ws, shift, affine)       # CPU, before the first GPU call
    m = copy.deepcopy(m).to(DEV)
    x = x64.to(DEV, dtype).requires_grad_(True)
    aff = torch.tensor(BLOCK_AFF, device=DEV) if affine else None
    y = m(x, aff)
    (y.float() * r64.to(DEV, torch.float32)).sum().backward()
    ty, tx, tp = (1e-3, 1e-3, 5e-3) if dtype == torch.float32 else (3e-2, 3e-2, 5e-2)
    errs = {"y": _rel(y, y64.numpy()), "dx": _rel(x.grad, dx64.numpy())}
    perrs = {}
    for name, p in m.named_parameters():
        assert p.grad is not None and name in grads, name
        if name.endswith("rel_pos_bias_affine_lin.bias"):
            perrs[name] = abs(float(p.grad) - float(grads[name])) / float(grads["attn.relative_position_bias_table"].abs().sum())
        else:
            perrs[name] = _rel(p.grad, grads[name].numpy())
    print(f"[{dtype} {res} ws {ws} affine {affine}]", {k: f"{v:.2e}" for k, v in {**errs, **perrs}.items()})
    assert errs["y"] < ty and errs["dx"] < tx, errs
    assert max(perrs.values()) < tp, perrs


@pytest.mark.parametrize("tag,vol", [("v24", (24, 24, 24)), ("v20", (20, 20, 20))])
def test_swin_encoder_vs_reference_golden(golden_dir, tag, vol):
    from medicalsemseg_amd.models.swin_unetr import SwinTransformerNNFormer
    g = _load(golden_dir, f"swin_encoder_{tag}.npz")
    m = SwinTransformerNNFormer(vol, (2, 2, 2), 1, 32, (2, 2), (2, 4), (6, 3), drop_path_rate=0.0,
                                compute_dtype=torch.float32)
    det_fill_(m, "enc")
    m = m.to(DEV)
    x = det_tensor("enc_x_" + tag, (2, 1) + vol).to(DEV)
    feats, _ = m((x, None, None))
    loss = 0
    for i, f in enumerate(feats):
        ref = g[f"out{i}"]
        got = f.permute(0, 4, 1, 2, 3)
        assert _rel(got, ref) < 1e-3, f"feature {i}"
        loss = loss + (got * det_tensor(f"enc_r{i}_" + tag, ref.shape).to(DEV)).sum()
    loss.backward()
    assert _rel(m.layers[0].blocks[1].attn.qkv.weight.grad, g["d_qkv_w"]) < 5e-3
    assert _rel(m.layers[0].blocks[1].attn.relative_position_bias_table.grad, g["d_table"]) < 5e-3
    assert _rel(m.layers[1].downsample.reduction.weight.grad[:8], g["d_merge_w"]) < 5e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swin_unetr_vs_oracle(dtype):
    """whole Swin-UNETR (reference-wired encoder + UNETR decoder) forward + DiceCE + backward vs the CPU oracle"""
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models import swin_unetr as P
    from oracle import swin as O
    from oracle.losses import dice_ce_loss
    torch.manual_seed(0)
    vol, hs = (32, 32, 32), 16
    kw = dict(patch_size=(2, 2, 2), in_chans=1, embed_dim=hs, depths=(2, 2), num_heads=(1, 2), window_size=(4, 4))
    ref = O.SwinUNETRCustom(O.SwinTransformerNNFormer(vol, **kw), 1, 3, hs, 2)
    enc = P.SwinTransformerNNFormer(vol, drop_path_rate=0.0, compute_dtype=dtype, **kw)
    net = P.SwinUNETRCustom(enc, 1, 3, vol, hs, (2, 2, 2), compute_dtype=dtype)
    sd = {k: v for k, v in ref.state_dict().items()}
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV)
    x = det_tensor("su_x", (2, 1) + vol)
    gl = torch.Generator().manual_seed(3)
    y = torch.randint(0, 3, (2, 1) + vol, generator=gl).float()
    out_ref = ref((x, None, None))
    loss_ref = dice_ce_loss(out_ref, y)
    loss_ref.backward()
    out = net((x.to(DEV), None, None))
    loss = DiceCELoss()(out, y.to(DEV))
    loss.backward()
    if dtype == torch.float32:
        np.testing.assert_allclose(out.detach().cpu().numpy(), out_ref.detach().numpy(), rtol=1e-4, atol=2e-4)
        assert abs(float(loss.detach()) - float(loss_ref.detach())) < 1e-4
    else:
        print(f"[bf16] Swin-UNETR 32^3: logits err/scale {_rel(out, out_ref.detach().numpy()):.3e}, |loss diff| "
              f"{abs(float(loss.detach()) - float(loss_ref.detach())):.2e}")
        assert _rel(out, out_ref.detach().numpy()) < BF16_GATES["swin32"][0]
        assert abs(float(loss.detach()) - float(loss_ref.detach())) < BF16_GATES["swin32"][1]
    pr = dict(ref.named_parameters())
    num = den = 0.0
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        gr = pr[name].grad
        num += float(((p.grad.cpu() - gr) ** 2).sum())
        den += float((gr ** 2).sum())
    tot = (num / den) ** 0.5
    print(f"[{dtype}] Swin-UNETR 32^3 whole-net grad rel-L2 {tot:.3e}")
    assert tot < (2e-3 if dtype == torch.float32 else BF16_GATES["swin32"][2]), f"whole-net grad rel L2 err {tot:.3e}"


def test_swin_official_encoder_vs_reference_golden(golden_dir):
    """product SwinViT (MONAI / official variant: padded 7-windows, clamped windows with the sliced 7^3 index,
    duplicated-sub-grid Linear patch merging, un-affine proj_out) against vectors of the REFERENCE's own
    swin_unetr_official.py; token grid 14 -> 7 -> 4 -> 2 -> 1"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.models.swin_unetr_official import _SwinViT
    g = _load(golden_dir, "swin_official_encoder.npz")
    vit = _SwinViT(1, 24, 7, (2, 2, 2, 2), (3, 6, 12, 24))
    det_fill_(vit, "swo_vit.")
    vit = vit.to(DEV)
    x = det_tensor("swo_x28", (1, 1, 28, 28, 28)).to(DEV)
    x_cl = torch.empty(1, 28, 28, 28, 1, device=DEV)
    hip.to_channels_last(x, x_cl)
    outs = vit(x_cl, True)
    loss = 0
    for i, o in enumerate(outs):
        got = o.permute(0, 4, 1, 2, 3)
        assert _rel(got, g[f"out{i}"]) < 1e-3, f"feature {i}"
        loss = loss + (got * det_tensor(f"swo_r{i}", g[f"out{i}"].shape).to(DEV)).sum()
    loss.backward()
    blk = vit.layers1[0].blocks[1]
    assert _rel(blk.attn.qkv.weight.grad, g["d_qkv_w"]) < 5e-3
    assert _rel(blk.attn.qkv.bias.grad, g["d_qkv_b"]) < 5e-3          # incl. the padded tokens' share
    assert _rel(blk.attn.relative_position_bias_table.grad, g["d_table"]) < 5e-3
    assert _rel(vit.layers1[0].downsample.reduction.weight.grad, g["d_merge_w"]) < 5e-3
    assert _rel(vit.layers2[0].blocks[1].attn.relative_position_bias_table.grad, g["d_table_l2"]) < 5e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swin_official_net_vs_reference_golden_and_oracle(golden_dir, dtype):
    """whole official Swin-UNETR (feature 24, 64^3): logits / gradients against the reference-file golden (fp32) and
    against the oracle restatement on random labels with DiceCE (both dtypes)"""
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models.swin_unetr_official import SwinUNETR
    from oracle import swin_official as O
    from oracle.losses import dice_ce_loss
    gn = _load(golden_dir, "swin_official_net.npz")
    ref = O.SwinUNETR((64, 64, 64), 1, 3, feature_size=24)
    det_fill_(ref, "swo_net.")
    net = SwinUNETR((64, 64, 64), 1, 3, feature_size=24, compute_dtype=dtype)
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(DEV)
    x = det_tensor("swo_x64", (1, 1, 64, 64, 64))
    out = net(x.to(DEV))                       # bare volume, as MONAI's inferer calls it
    if dtype == torch.float32:
        assert _rel(out[:, :, ::2, ::2, ::2], gn["logits_s2"]) < 2e-4
        (out * det_tensor("swo_ry", tuple(out.shape)).to(DEV)).sum().backward()
        assert _rel(net.out.conv.conv.weight.grad, gn["d_out_w"]) < 2e-3
        assert _rel(net.encoder1.layer.conv1.conv.weight.grad[:12], gn["d_enc1_w"]) < 2e-3
        assert _rel(net.swinViT.patch_embed.proj.weight.grad, gn["d_patch_w"]) < 5e-3
        assert _rel(net.swinViT.layers4[0].blocks[0].mlp.linear1.weight.grad[:96, :96], gn["d_l4_fc"]) < 5e-3
        for p in net.parameters():
            p.grad = None
    gl = torch.Generator().manual_seed(3)
    y = torch.randint(0, 3, (1, 1, 64, 64, 64), generator=gl).float()
    out_ref = ref((x, None, None))
    loss_ref = dice_ce_loss(out_ref, y)
    loss_ref.backward()
    out = net((x.to(DEV), None, None))
    loss = DiceCELoss()(out, y.to(DEV))
    loss.backward()
    err = _rel(out, out_ref.detach().numpy())
    pr = dict(ref.named_parameters())
    num = den = 0.0
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        num += float(((p.grad.cpu() - pr[name].grad) ** 2).sum())
        den += float((pr[name].grad ** 2).sum())
    tot = (num / den) ** 0.5
    print(f"[{dtype}] official Swin-UNETR 64^3: logits err/scale {err:.3e}, grad rel-L2 {tot:.3e}")
    if dtype == torch.float32:
        assert err < 2e-4 and abs(float(loss.detach()) - float(loss_ref.detach())) < 1e-4 and tot < 2e-3
    else:
        print(f"[bf16] official Swin-UNETR 64^3 |loss diff| {abs(float(loss.detach()) - float(loss_ref.detach())):.2e}")
        # measured 9.1e-3 / 1.9e-2: gates at about twice that
        assert err < BF16_GATES["official64"][0] and abs(float(loss.detach()) - float(loss_ref.detach())) < BF16_GATES["official64"][1] \
            and tot < BF16_GATES["official64"][2]


@pytest.mark.parametrize("R,ws,heads,C,shift,bws", [(12, 7, 3, 48, 3, 7), (14, 7, 4, 64, 0, 7), (9, 7, 3, 48, 3, 7),
                                                       (6, 6, 24, 384, 0, 7), (4, 4, 12, 192, 0, 7)])
def test_window7_attention_mfma_equals_vector_kernels(monkeypatch, R, ws, heads, C, shift, bws):
    """343-token windows (MONAI Swin-UNETR): the bf16 MFMA kernels (11 key tiles, online-softmax chunks, 12-bit bias
    codes) against the exact-fp32-math vector kernels on the same bf16 operands, forward and backward, with padding
    (12 -> 14, 9 -> 14) and the shift mask"""
    from medicalsemseg_amd import hip
    torch.manual_seed(7)
    qkv = (torch.randn(2, R, R, R, 3 * C, device=DEV) * 0.7).bfloat16()
    qb = torch.randn(3 * C, device=DEV) * 0.3
    tab = torch.randn((2 * bws - 1) ** 3, heads, device=DEV) * 0.3     # bws > ws: clamped window, sliced 7^3 index
    dout = torch.randn(2, R, R, R, C, device=DEV).bfloat16()
    res = []
    for no_mfma in (False, True):
        if no_mfma:
            monkeypatch.setenv("MSSEG_ATTN_NO_MFMA", "1")
        else:
            monkeypatch.delenv("MSSEG_ATTN_NO_MFMA", raising=False)
        out = torch.empty(2, R, R, R, C, device=DEV, dtype=torch.bfloat16)
        lse = hip.window_attention_fwd(qkv, qb, tab, out, heads, ws, shift, bws)
        dqkv = torch.empty_like(qkv)
        dtab = torch.zeros_like(tab)
        hip.window_attention_bwd(qkv, qb, tab, out, lse, dout, dqkv, dtab, heads, ws, shift, bws)
        res.append((out.float(), lse.clone(), dqkv.float(), dtab.clone()))
    monkeypatch.delenv("MSSEG_ATTN_NO_MFMA", raising=False)
    (o0, l0, d0, t0), (o1, l1, d1, t1) = res
    assert float((o0 - o1).abs().max()) / float(o1.abs().max()) < 2e-2
    assert float((l0 - l1).abs().max()) < 2e-2
    assert float((d0 - d1).norm() / d1.norm()) < 3e-2
    assert float((t0 - t1).norm() / t1.norm()) < 3e-2


def test_drop_path_residual_add_vs_reference_golden(golden_dir):
    """stochastic depth folded into the residual-add kernel: with the reference's own mask (recovered from the
    DropPath(0.2) golden of /root/reference/models/layers/drop_path.py under seed 7), shortcut + drop_path(branch)
    equals the reference's arithmetic, forward and backward; eval mode is the plain add"""
    from medicalsemseg_amd import ops
    g = _load(golden_dir, "layers_ref.npz")
    x, y_ref = torch.from_numpy(g["dp_x"]), torch.from_numpy(g["dp_y"])            # [16, 5, 7]
    kept = (y_ref.abs().reshape(16, -1).max(1).values > 0).float()
    assert 0 < float(kept.sum()) < 16
    B = 16
    branch = torch.zeros(B, 2, 2, 2, 40)
    branch.reshape(B, -1)[:, :35] = x.reshape(B, -1)
    shortcut = det_tensor("dp_short", (B, 2, 2, 2, 40))
    for dtype in (torch.float32, torch.bfloat16):
        a = shortcut.to(DEV, dtype).requires_grad_(True)
        b = branch.to(DEV, dtype).requires_grad_(True)
        out = ops.add(a, b, (kept / 0.8).to(DEV))
        want = shortcut.to(dtype).float() + torch.zeros_like(branch).copy_(branch.to(dtype).float())* (kept / 0.8).view(B, 1, 1, 1, 1)
        tol = 1e-6 if dtype == torch.float32 else 1e-2
        # bf16: one rounding of the sum (half an ulp = 2^-9 relative)
        assert float(((out.float().cpu() - want).abs() / want.abs().clamp(min=1.0)).max()) < (1e-6 if dtype == torch.float32 else 2.0 ** -8)
        if dtype == torch.float32:   # the golden itself: branch part of the sum == reference DropPath output
            got_dp = (out.float().cpu() - shortcut).reshape(B, -1)[:, :35].reshape(16, 5, 7)
            assert float((got_dp - y_ref).abs().max()) < 1e-5
        r = det_tensor("dp_r", tuple(out.shape)).to(DEV, dtype)
        (out * r).sum().backward()
        assert torch.equal(a.grad, r)
        gw = r.float().cpu() * (kept / 0.8).view(B, 1, 1, 1, 1)
        assert float(((b.grad.float().cpu() - gw).abs() / gw.abs().clamp(min=1.0)).max()) < (1e-6 if dtype == torch.float32 else 2.0 ** -8)
    # a training-mode block draws its own mask; eval mode applies none
    from medicalsemseg_amd.models.swin_unetr import _Block
    blk = _Block(48, (6, 6, 6), 3, 6, 0, 4.0, True, 0.5).to(DEV)
    xin = torch.randn(4, 6, 6, 6, 48, device=DEV)
    blk.eval()
    e1, e2 = blk(xin), blk(xin)
    assert torch.equal(e1, e2)
    blk.train()
    blk.dp_mask = torch.tensor([1.0, 0.0, 1.0, 0.0])
    t = blk(xin)
    assert torch.equal(t[1], xin[1]) and torch.equal(t[3], xin[3])      # dropped samples keep the shortcut only
    assert not torch.equal(t[0], e1[0])                                 # kept samples: branch scaled by 1 / keep


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swinception_encoder_vs_reference_golden(golden_dir, dtype):
    """SwInception encoder (Inception-head MLP) against the reference's own
    models/backbones/swinception.py (tests/golden/swinception_encoder.npz): training-mode features, gradient probes through
    every branch (4- / 25- / 8- / 51-channel convolutions run zero-padded to multiples of 8), running statistics,
    eval-mode features; the weights arrive through the reference-shaped state dict"""
    from medicalsemseg_amd.models.swin_unetr import SwInception
    from oracle import swin as OW
    g = _load(golden_dir, "swinception_encoder.npz")
    vol = (24, 24, 24)
    ref = OW.SwinTransformerNNFormer(vol, (2, 2, 2), 1, 32, (2, 2), (2, 4), (6, 3), mlp="inception")
    det_fill_(ref, "si")
    m = SwInception(vol, (2, 2, 2), 1, 32, (2, 2), (2, 4), (6, 3), drop_path_rate=0.0, compute_dtype=dtype)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).train()
    x = det_tensor("si_x", (2, 1) + vol).to(DEV)
    feats, _ = m((x, None, None))
    tol_f, tol_g = (1e-3, 5e-3) if dtype == torch.float32 else (6e-2, 1.5e-1)   # bf16: drift through 44 BatchNorm stages
    loss = 0
    for i, f in enumerate(feats):
        got = f.permute(0, 4, 1, 2, 3)
        assert _rel(got, g[f"out{i}"]) < tol_f, f"feature {i}: {_rel(got, g[f'out{i}']):.3e}"
        loss = loss + (got.float() * det_tensor(f"si_r{i}", g[f"out{i}"].shape).to(DEV)).sum()
    loss.backward()
    mlp = m.layers[0].blocks[1].mlp
    b = mlp.branches
    fcw = lambda q: q.fc.weight.grad.view(q.fc.weight.shape[0], 5, -1)[:, :, :q.branch].reshape(q.fc.weight.shape[0], -1)
    probes = {"d_b1_w": b[0].branch1x1.conv.weight.grad[:25, :32], "d_b3_2_w": b[1].branch3x3_2.conv.weight.grad[:25, :4],
              "d_b5_2_w": b[2].branch3x3dbl_2.conv.weight.grad[:4, :4], "d_b7_1_w": b[3].branch3x3trpl_1.conv.weight.grad[:4, :32],
              "d_b7_4_bn_w": b[3].branch3x3trpl_4.bn.weight.grad[:25], "d_b7_4_bn_b": b[3].branch3x3trpl_4.bn.bias.grad[:25],
              "d_pool_w": b[4].branch_pool_2.conv.weight.grad[:25, :32], "d_fc_w": fcw(mlp), "d_fc_b": mlp.fc.bias.grad,
              "d_fc_w_l1": fcw(m.layers[1].blocks[0].mlp)}
    errs = {k: _rel(t, g[k]) for k, t in probes.items()}
    print(f"[{dtype}] SwInception 24^3 gradient errors:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < tol_g, errs
    # every gradient that lands on a padding entry is exactly zero (so the padding stays zero under AdamW)
    w = b[2].branch3x3dbl_2.conv.weight.grad
    assert float(w[4:].abs().max()) == 0.0 and float(w[:, 4:].abs().max()) == 0.0
    assert float(b[3].branch3x3trpl_4.bn.weight.grad[25:].abs().max()) == 0.0
    assert float(mlp.fc.weight.grad.view(32, 5, -1)[:, :, 25:].abs().max()) == 0.0
    bn = b[2].branch3x3dbl_3.bn
    if dtype == torch.float32:
        assert np.allclose(bn.running_mean[:25].cpu().numpy(), g["rm"], atol=1e-4)
        assert np.allclose(bn.running_var[:25].cpu().numpy(), g["rv"], atol=1e-4)
    m.eval()
    with torch.no_grad():
        ef, _ = m((x, None, None))
    for i, f in enumerate(ef):
        assert _rel(f.permute(0, 4, 1, 2, 3), g[f"eval{i}"]) < tol_f, i


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swindepth_encoder_vs_reference_golden(golden_dir, dtype):
    """SwinDepth encoder (depthwise-conv + BatchNorm MLP) against the reference's own
    models/backbones/swindepth.py (tests/golden/swindepth_encoder.npz): training-mode features and gradients,
    running statistics, eval-mode features"""
    from medicalsemseg_amd.models.swin_unetr import SwinDepth
    g = _load(golden_dir, "swindepth_encoder.npz")
    vol = (24, 24, 24)
    m = SwinDepth(vol, (2, 2, 2), 1, 32, (2, 2), (2, 4), (6, 3), drop_path_rate=0.0, compute_dtype=dtype)
    det_fill_(m, "sd")
    m = m.to(DEV).train()
    x = det_tensor("sd_x", (2, 1) + vol).to(DEV)
    feats, _ = m((x, None, None))
    tol_f, tol_g = (1e-3, 5e-3) if dtype == torch.float32 else (6e-2, 1.5e-1)   # bf16: drift through 12 BatchNorm stages
    loss = 0
    for i, f in enumerate(feats):
        got = f.permute(0, 4, 1, 2, 3)
        assert _rel(got, g[f"out{i}"]) < tol_f, f"feature {i}: {_rel(got, g[f'out{i}']):.3e}"
        loss = loss + (got.float() * det_tensor(f"sd_r{i}", g[f"out{i}"].shape).to(DEV)).sum()
    loss.backward()
    mlp = m.layers[0].blocks[1].mlp
    # a conv bias in front of a training-mode BatchNorm has a zero gradient: rounding noise on both sides
    zero_tol = 1e-3 if dtype == torch.float32 else 2e-2      # bf16: the sum of 3456 rounded gradient values per channel
    assert float(mlp.dwc2.bias.grad.abs().max()) < zero_tol * float(np.abs(g["d_dwc2_w"]).max()) and np.abs(g["d_dwc2_b"]).max() < 1e-3
    errs = {k: _rel(t, g[k]) for k, t in (("d_dwc2_w", mlp.dwc2.weight.grad),
                                           ("d_bn2_w", mlp.bn2.weight.grad), ("d_bn2_b", mlp.bn2.bias.grad),
                                           ("d_fc1_w", mlp.fc1.weight.grad),
                                           ("d_fc2_w", m.layers[1].blocks[0].mlp.fc2.weight.grad))}
    print(f"[{dtype}] SwinDepth 24^3 gradient errors:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < tol_g, errs
    if dtype == torch.float32:
        assert np.allclose(mlp.bn3.running_mean.cpu().numpy(), g["rm"], atol=1e-4)
        assert np.allclose(mlp.bn3.running_var.cpu().numpy(), g["rv"], atol=1e-4)
    m.eval()
    with torch.no_grad():
        fe, _ = m((x, None, None))
    for i, f in enumerate(fe):
        assert _rel(f.permute(0, 4, 1, 2, 3), g[f"eval{i}"]) < tol_f, f"eval feature {i}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_segformer3d_vs_reference_golden(golden_dir, dtype):
    """SegFormer3D (MixVisionTransformer + SegFormerHeadOfficial) against the reference's own classes
    (tests/golden/segformer3d_ref.npz): training-mode logits, encoder features, gradient probes through every new kernel
    (gather conv k7 s4, spatial-reduction conv + its input gradient, few-key attention, depthwise conv, trilinear
    interpolation, BatchNorm), running statistics, eval-mode logits"""
    from medicalsemseg_amd.models.segformer3d import MixVisionTransformer, SegFormerHeadOfficial
    from tests.golden_util import SEGFORMER_CFG as c, probe
    g = _load(golden_dir, "segformer3d_ref.npz")
    enc = MixVisionTransformer(c["vol"], 16, 1, c["embed_dim"], c["num_heads"], (4, 4, 4, 4), True, 0.0, c["depths"],
                               (8, 4, 2, 1), compute_dtype=dtype)
    net = SegFormerHeadOfficial(enc, [c["embed_dim"] * 2 ** i for i in range(4)], c["classes"], 0.0, c["embedding_dim"],
                                compute_dtype=dtype)
    det_fill_(net, "segf.")
    net = net.to(DEV).train()
    x = det_tensor("segf_x", (2, 1) + c["vol"]).to(DEV)
    sub = lambda t: t[:, :, ::2, ::2, ::2]
    feats = enc((x, None, None))
    tf, tg = (1e-3, 5e-3) if dtype == torch.float32 else (5e-2, 1.5e-1)
    ef = {"feat1": _rel(sub(feats[1].permute(0, 4, 1, 2, 3)), g["feat1_s2"])}
    for i in (2, 3, 4):
        ef[f"feat{i}"] = _rel(feats[i].permute(0, 4, 1, 2, 3), g[f"feat{i}"])
    y = net((x, None, None))
    ef["logits"] = _rel(sub(y), g["logits_s2"])
    (y.float() * det_tensor("segf_r", tuple(y.shape)).to(DEV)).sum().backward()
    P = dict(net.named_parameters())
    eg = {}
    for k in [k[2:] for k in g.files if k.startswith("g:")]:
        w = g["g:" + k]
        got = probe(P[k].grad).float().cpu().numpy()
        if np.linalg.norm(w) < 1e-3:      # a bias whose effect the training-mode BatchNorm removes: zero up to rounding noise
            # (bf16: a sum of ~10^4 rounded gradient values per channel; the realisation moves with any change of rounding order upstream)
            assert np.linalg.norm(got) < (1e-2 if dtype == torch.float32 else 2.0), k
            continue
        eg[k] = float(np.linalg.norm(got - w) / np.linalg.norm(w))
    print(f"[{dtype}] SegFormer3D 64^3 forward errors:", {k: f"{v:.2e}" for k, v in ef.items()})
    print(f"[{dtype}] SegFormer3D 64^3 gradient probe rel-L2:", {k: f"{v:.2e}" for k, v in eg.items()})
    assert max(ef.values()) < tf, ef
    assert max(eg.values()) < tg, eg
    if dtype == torch.float32:
        assert np.allclose(net.linear_fuse.bn.running_mean.cpu().numpy(), g["rm"], atol=1e-4)
        assert np.allclose(net.linear_fuse.bn.running_var.cpu().numpy(), g["rv"], atol=1e-4)
    net.eval()
    with torch.no_grad():
        assert _rel(sub(net((x, None, None))), g["logits_eval_s2"]) < tf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swin_segformer_vs_reference_golden(golden_dir, dtype):
    """'SwinSegFormer' (SwinTransformerNNFormer + the progressive-fusion SegFormerHead; /root/reference/models/
    model_builder.py:173-189, models/segmentors/segformer_head.py:40-121) against the reference's own classes
    (tests/golden/swin_segformer_ref.npz): training-mode logits, gradient probes through encoder, every fusion level and the
    prediction conv, the four BatchNorms' running statistics, eval-mode logits.  The product applies dropout + prediction
    conv before the final upsampling (they commute with it): fp32 must still meet rtol 1e-4-level agreement."""
    from medicalsemseg_amd.models.segformer3d import SegFormerHead
    from medicalsemseg_amd.models.swin_unetr import SwinTransformerNNFormer
    from tests.golden_util import SWIN_SEGFORMER_CFG as c, probe
    g = _load(golden_dir, "swin_segformer_ref.npz")
    enc = SwinTransformerNNFormer(c["vol"], (2, 2, 2), 1, c["embed_dim"], tuple(c["depths"]), tuple(c["num_heads"]),
                                  tuple(c["window_size"]), drop_path_rate=0.0, compute_dtype=dtype)
    net = SegFormerHead(enc, [c["embed_dim"] * 2 ** i for i in range(5)], c["classes"], 0.0, c["embedding_dim"],
                        compute_dtype=dtype)
    det_fill_(net, "swsf.")
    net = net.to(DEV).train()
    x = det_tensor("swsf_x", (2, 1) + c["vol"]).to(DEV)
    y = net((x, None, None))
    e_log = _rel(y, g["logits"])
    (y.float() * det_tensor("swsf_r", tuple(y.shape)).to(DEV)).sum().backward()
    P = dict(net.named_parameters())
    eg = {}
    for k in c["probes"]:
        w = g["g:" + k]
        got = probe(P[k].grad).float().cpu().numpy()
        eg[k] = float(np.linalg.norm(got - w) / np.linalg.norm(w))
    print(f"[{dtype}] SwinSegFormer 32^3 logits err/scale {e_log:.2e}; gradient probe rel-L2:", {k: f"{v:.2e}" for k, v in eg.items()})
    tf, tg = (2e-4, 5e-3) if dtype == torch.float32 else (5e-2, 1.5e-1)
    assert e_log < tf and max(eg.values()) < tg, (e_log, eg)
    if dtype == torch.float32:
        for i in range(4):
            bn = getattr(net, f"linear_fuse_{i}").bn
            assert np.allclose(bn.running_mean.cpu().numpy(), g[f"rm{i}"], atol=1e-4), i
            assert np.allclose(bn.running_var.cpu().numpy(), g[f"rv{i}"], atol=1e-4), i
    net.eval()
    with torch.no_grad():
        e_eval = _rel(net((x, None, None)), g["logits_eval"])
    print(f"[{dtype}] SwinSegFormer eval logits err/scale {e_eval:.2e}")
    assert e_eval < tf
