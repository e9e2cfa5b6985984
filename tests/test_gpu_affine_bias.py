"""GPU tests of the spacing-conditioned relative position bias (`--rel_pos_bias_affine`): window attention and the three
Swin encoder families against the reference's own modules (tests/golden/*affine*, tools/gen_golden_affine.py), exact
identities of the fold, determinism of the table-gradient path, the gradient-buffer protocol and the engine paths."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden_util import det_fill_, det_tensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TOKEN_STRIDE = 4          # the attention fixtures keep every fourth token of every window
AFF = [[1.5, 0.8, 2.0], [-0.7, 1.25, 3.0]]
ENC = ((2, 2, 2), 1, 32, (2, 2), (2, 4), (6, 3))      # patch, in_chans, embed_dim, depths, heads, windows of the fixtures


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _rel(a, b):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else a
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


class _AffineParams:
    """det_fill_ over the affine parameters of a module only (det_fill_ draws each parameter from its own name)"""

    def __init__(self, m):
        self.m = m

    def named_parameters(self):
        return [(n, p) for n, p in self.m.named_parameters() if "rel_pos_bias_affine" in n]


def _windows_to_volume(xw, ws, shift):
    """[2 * 8, N, C] windows of two SHIFTED (2ws)^3 grids -> unshifted volumes [2, 2ws, 2ws, 2ws, C]"""
    from oracle.swin import window_reverse
    C = xw.shape[-1]
    vol = window_reverse(xw.reshape(16, ws, ws, ws, C), ws, 2 * ws, 2 * ws, 2 * ws)
    return torch.roll(vol, shifts=(shift, shift, shift), dims=(1, 2, 3))


def _volume_to_windows(vol, ws, shift):
    from oracle.swin import window_partition
    v = torch.roll(vol, shifts=(-shift, -shift, -shift), dims=(1, 2, 3))
    return window_partition(v, ws).reshape(16, ws ** 3, -1)


def _affine_grads(attn):
    return (attn.relative_position_bias_table.grad, attn.rel_pos_bias_affine_emb.grad,
            attn.rel_pos_bias_affine_lin.weight.grad, attn.rel_pos_bias_affine_lin.bias.grad)


# ------------------------------------------------------------------------------------------------------------------
# 1. window attention against the reference
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tag,dim,ws,heads", [("h3w6", 48, 6, 3), ("h24w3", 384, 3, 24)])
def test_window_attention_affine_vs_reference_golden(golden_dir, dtype, tag, dim, ws, heads):
    """two samples x 8 windows with different spacings (one negative): fp32 runs the vector kernels, bf16 the MFMA kernels
    with the workspace table gradient; gates as test_window_attention_vs_reference_golden, the emb / lin gradients under
    the table's.  lin.b's gradient is the sum of all dS, zero up to rounding (every softmax row's dS sums to 0): it is gated
    in absolute terms against the L1 mass of the table gradient it sums."""
    from medicalsemseg_amd import ops
    from medicalsemseg_amd.models.swin_unetr import _WindowAttention
    g = _load(golden_dir, f"swin_attn_affine_{tag}.npz")
    m = _WindowAttention(dim, ws, heads, True, rel_pos_bias_affine=True)
    det_fill_(m, "attn_aff_" + tag)
    m = m.to(DEV)
    N = ws ** 3
    xw = det_tensor("attn_aff_x_" + tag, (16, N, dim))
    rw = det_tensor("attn_aff_r_" + tag, (16, N, dim))
    aff = torch.tensor(g["affine"]).to(DEV)
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    tol_p = 1e-3 if dtype == torch.float32 else 5e-2
    for mk, shift in (("nomask", 0), ("mask", ws // 2)):
        x = _windows_to_volume(xw, ws, shift).to(DEV, dtype).requires_grad_(True)
        r = _windows_to_volume(rw, ws, shift).to(DEV, dtype)
        for p in m.parameters():
            p.grad = None
        qkv = ops.linear(x, m.qkv.weight, m.qkv.bias)
        y = ops.WindowAttnAffineFn.apply(qkv, m.qkv.bias, m.relative_position_bias_table, m.rel_pos_bias_affine_emb,
                                         m.rel_pos_bias_affine_lin.weight, m.rel_pos_bias_affine_lin.bias, aff, heads, ws, shift)
        y = ops.linear(y, m.proj.weight, m.proj.bias)
        (y.float() * r.float()).sum().backward()
        yw = _volume_to_windows(y.detach().float().cpu(), ws, shift)[:, ::TOKEN_STRIDE]
        dxw = _volume_to_windows(x.grad.float().cpu(), ws, shift)[:, ::TOKEN_STRIDE]
        dtab, demb, dlw, dlb = _affine_grads(m)
        errs = {"y": _rel(yw, g[f"y_{mk}"]), "dx": _rel(dxw, g[f"dx_{mk}"])}
        perrs = {"dtable": _rel(dtab, g[f"dtable_{mk}"]), "demb": _rel(demb, g[f"demb_{mk}"]),
                 "dlin_w": _rel(dlw, g[f"dlin_w_{mk}"]),
                 "dlin_b": float(abs(float(dlb) - float(g[f"dlin_b_{mk}"][0])) / np.abs(g[f"dtable_{mk}"]).sum())}
        print(f"[{dtype} {tag} {mk}]", {k: f"{v:.2e}" for k, v in {**errs, **perrs}.items()})
        assert max(errs.values()) < tol, errs
        assert max(perrs.values()) < tol_p, perrs


# ------------------------------------------------------------------------------------------------------------------
# 2. encoders against the reference
# ------------------------------------------------------------------------------------------------------------------
def _encoder_vs_golden(m, g, x, rtag, tol_f=1e-3, tol_g=5e-3):
    """features and the table / emb / lin gradients of layer 0's shifted block (the volume enters the encoder through a
    layout kernel: no input gradient here, as in test_swin_encoder_vs_reference_golden)"""
    aff = torch.tensor(g["affine"]).to(DEV)
    feats, _ = m((x.to(DEV), None, aff))
    loss = 0
    for i, f in enumerate(feats):
        got = f.permute(0, 4, 1, 2, 3)
        assert _rel(got, g[f"out{i}"]) < tol_f, f"feature {i}: {_rel(got, g[f'out{i}']):.3e}"
        loss = loss + (got.float() * det_tensor(f"{rtag}{i}", g[f"out{i}"].shape).to(DEV)).sum()
    loss.backward()
    dtab, demb, dlw, dlb = _affine_grads(m.layers[0].blocks[1].attn)
    errs = {"d_table": _rel(dtab, g["d_table"]), "d_emb": _rel(demb, g["d_emb"]), "d_lin_w": _rel(dlw, g["d_lin_w"]),
            "d_lin_b": float(abs(float(dlb) - float(g["d_lin_b"][0])) / np.abs(g["d_table"]).sum())}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < tol_g, errs


def test_swin_encoder_affine_vs_reference_golden_padded_grid(golden_dir):
    """20^3 volume = a 10^3 token grid under window 6: padded windows carry the per-sample bias too"""
    from medicalsemseg_amd.models.swin_unetr import SwinTransformerNNFormer
    g = _load(golden_dir, "swin_encoder_affine_v20.npz")
    m = SwinTransformerNNFormer((20,) * 3, *ENC, drop_path_rate=0.0, compute_dtype=torch.float32, rel_pos_bias_affine=True)
    det_fill_(m, "enc_aff")
    _encoder_vs_golden(m.to(DEV), g, det_tensor("enc_aff_x", (2, 1, 20, 20, 20)), "enc_aff_r")


def test_swindepth_encoder_affine_vs_reference_golden(golden_dir):
    from medicalsemseg_amd.models.swin_unetr import SwinDepth
    g = _load(golden_dir, "swindepth_encoder_affine.npz")
    m = SwinDepth((24,) * 3, *ENC, drop_path_rate=0.0, compute_dtype=torch.float32, rel_pos_bias_affine=True)
    det_fill_(m, "sd_aff")
    _encoder_vs_golden(m.to(DEV).train(), g, det_tensor("sd_aff_x", (2, 1, 24, 24, 24)), "sd_aff_r")


def test_swinception_encoder_affine_vs_reference_golden(golden_dir):
    """the Inception head computes zero-padded: the weights arrive through the reference-shaped state dict of the oracle's
    module (as in test_swinception_encoder_vs_reference_golden), the affine parameters by their own names"""
    from medicalsemseg_amd.models.swin_unetr import SwInception
    from oracle import swin as OW
    g = _load(golden_dir, "swinception_encoder_affine.npz")
    ref = OW.SwinTransformerNNFormer((24,) * 3, *ENC, mlp="inception")
    det_fill_(ref, "si_aff")
    m = SwInception((24,) * 3, *ENC, drop_path_rate=0.0, compute_dtype=torch.float32, rel_pos_bias_affine=True)
    missing, unexpected = m.load_state_dict(ref.state_dict(), strict=False)
    assert not unexpected and missing and all("rel_pos_bias_affine" in k for k in missing)
    det_fill_(_AffineParams(m), "si_aff")
    _encoder_vs_golden(m.to(DEV).train(), g, det_tensor("si_aff_x", (2, 1, 24, 24, 24)), "si_aff_r", tol_g=1e-2)


# ------------------------------------------------------------------------------------------------------------------
# 3. exact identities (bf16: MFMA kernels, workspace table gradient)
# ------------------------------------------------------------------------------------------------------------------
def _pair_models(dtype=torch.bfloat16, seed=0):
    """flag-on and flag-off encoders with the same shared weights"""
    from medicalsemseg_amd.models.swin_unetr import SwinTransformerNNFormer
    torch.manual_seed(seed)
    on = SwinTransformerNNFormer((24,) * 3, *ENC, drop_path_rate=0.0, compute_dtype=dtype, rel_pos_bias_affine=True)
    det_fill_(on, "exact")
    off = SwinTransformerNNFormer((24,) * 3, *ENC, drop_path_rate=0.0, compute_dtype=dtype)
    missing, unexpected = off.load_state_dict(on.state_dict(), strict=False)
    assert not missing and all("rel_pos_bias_affine" in k for k in unexpected)
    return on.to(DEV), off.to(DEV)


def _run(m, x, aff, seed=1):
    """features, the gradient that reaches the Swin layers' input (the patch embedding's output: the volume itself enters
    through a layout kernel) and every parameter gradient"""
    for p in m.parameters():
        p.grad = None
    feats, _ = m((x, None, aff))
    feats[0].retain_grad()
    loss = sum((f.float() * det_tensor(f"exact_r{i}_{seed}", f.shape).to(DEV)).sum() for i, f in enumerate(feats[1:]))
    loss.backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return [f.detach().clone() for f in feats], feats[0].grad.clone(), grads


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("B", [1, 2])
def test_affine_none_and_zero_affine_parameters_equal_flag_off(B):
    """(a) affine=None with the flag on runs the flag-off path; (b) emb = 0 and lin = 0 fold to the plain table: outputs,
    input gradient and the shared parameter gradients are the flag-off model's bit for bit.  The table gradient of (b)
    is compared at B = 1, where the per-sample window groups are the flag-off groups."""
    on, off = _pair_models()
    x = det_tensor(f"exact_x{B}", (B, 1, 24, 24, 24)).to(DEV)
    aff = torch.tensor(AFF[:B], device=DEV)
    f0, dx0, g0 = _run(off, x, None)
    f1, dx1, g1 = _run(on, x, None)
    assert _same(f0, f1) and torch.equal(dx0, dx1)
    assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    with torch.no_grad():
        for n, p in on.named_parameters():
            if "rel_pos_bias_affine" in n:
                p.zero_()
    f2, dx2, g2 = _run(on, x, aff)
    assert _same(f0, f2) and torch.equal(dx0, dx2)
    for k in g0:
        if B == 1 or "relative_position_bias_table" not in k:
            assert torch.equal(g0[k], g2[k]), k
    # and the term does act once the parameters are non-zero
    det_fill_(_AffineParams(on), "exact")
    f3, _, _ = _run(on, x, aff)
    assert not torch.equal(f0[1], f3[1])


def test_one_affine_row_equals_the_row_repeated_and_samples_swap():
    """A = 1 (sliding-window inference) equals that row given once per sample; swapping two samples together with their
    affine rows swaps the features"""
    on, _ = _pair_models()
    det_fill_(_AffineParams(on), "exact")
    x = det_tensor("exact_x2", (2, 1, 24, 24, 24)).to(DEV)
    row = torch.tensor(AFF[1:], device=DEV)
    fa, dxa, ga = _run(on, x, row)
    fb, dxb, gb = _run(on, x, row.repeat(2, 1))
    assert _same(fa, fb) and torch.equal(dxa, dxb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    aff = torch.tensor(AFF, device=DEV)
    on.eval()
    with torch.no_grad():
        f, _ = on((x, None, aff))
        fs, _ = on((x[[1, 0]].contiguous(), None, aff[[1, 0]].contiguous()))
    assert all(torch.equal(u[[1, 0]], v) for u, v in zip(f, fs))
    assert not torch.equal(f[1][0], f[1][1])
    with pytest.raises(ValueError, match="do not divide"):
        on((torch.cat([x, x[:1]]), None, aff))


# ------------------------------------------------------------------------------------------------------------------
# 4. determinism, 5. gradient-buffer protocol
# ------------------------------------------------------------------------------------------------------------------
def test_affine_parameter_gradients_are_bit_identical_run_to_run():
    on, _ = _pair_models()
    det_fill_(_AffineParams(on), "exact")
    x = det_tensor("exact_x2", (2, 1, 24, 24, 24)).to(DEV)
    aff = torch.tensor(AFF, device=DEV)
    _, _, g1 = _run(on, x, aff)
    _, _, g2 = _run(on, x, aff)
    keys = [k for k in g1 if "relative_position_bias_table" in k or "rel_pos_bias_affine" in k]
    assert len(keys) == 4 * 4
    for k in keys:
        assert torch.equal(g1[k], g2[k]), k
    assert float(g1["layers.0.blocks.1.attn.rel_pos_bias_affine_emb"].abs().max()) > 0


def test_two_backward_passes_accumulate_each_affine_gradient():
    """the second backward adds into every gradient buffer (table, emb, lin.w, lin.b each with its own flag): the sum of the
    two single-pass gradients, bit for bit"""
    on, _ = _pair_models()
    det_fill_(_AffineParams(on), "exact")
    aff = torch.tensor(AFF, device=DEV)
    xs = [det_tensor(f"exact_acc{i}", (2, 1, 24, 24, 24)).to(DEV) for i in range(2)]
    single = [_run(on, x, aff, seed=i)[2] for i, x in enumerate(xs)]
    for p in on.parameters():
        p.grad = None
    for i, x in enumerate(xs):
        feats, _ = on((x, None, aff))
        sum((f.float() * det_tensor(f"exact_r{j}_{i}", f.shape).to(DEV)).sum() for j, f in enumerate(feats[1:])).backward()
    for n, p in on.named_parameters():
        if "relative_position_bias_table" in n or "rel_pos_bias_affine" in n:
            assert torch.equal(p.grad, single[0][n] + single[1][n]), n


def test_lazy_zero_grad_equals_zero_filled_gradients_with_affine(monkeypatch):
    """FlatAdamW's lazy zero_grad (first kernel in an epoch overwrites) against the zero-filled buffer with accumulating
    kernels (MSSEG_EAGER_ZERO_GRAD=1), three clipped steps, the second with two backward passes: same parameters bit for bit"""
    from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay

    def run(eager):
        if eager:
            monkeypatch.setenv("MSSEG_EAGER_ZERO_GRAD", "1")
        else:
            monkeypatch.delenv("MSSEG_EAGER_ZERO_GRAD", raising=False)
        on, _ = _pair_models()
        det_fill_(_AffineParams(on), "exact")
        opt = FlatAdamW(add_weight_decay(on, 1e-5), lr=1e-3)
        aff = torch.tensor(AFF, device=DEV)
        for it in range(3):
            for rep in range(2 if it == 1 else 1):
                x = det_tensor(f"lazy_x{it}_{rep}", (2, 1, 24, 24, 24)).to(DEV)
                feats, _ = on((x, None, aff))
                sum((f.float() * det_tensor(f"lazy_r{j}", f.shape).to(DEV)).sum() for j, f in enumerate(feats)).backward()
            opt.clip_grad_norm_(1.0)
            opt.step()
            opt.zero_grad()
        return opt.flat_param.clone()

    lazy, eager = run(False), run(True)
    assert torch.equal(lazy, eager)


# ------------------------------------------------------------------------------------------------------------------
# 6. engine
# ------------------------------------------------------------------------------------------------------------------
_ENGINE_ARGS = ("--model nnFormerUNETR --output_dim 2 --vol_size 48 --patch_size 2 --hidden_dim 32 --depths 2 2 --num_heads 2 4 "
                "--window_size 6 3 --qkv_bias --gradient_clipping 1.0 --rel_pos_bias_affine")


class _SpacedLoader:
    """SyntheticLoader batches whose original affine has the diagonal of a non-isotropic, flipped spacing"""

    def __init__(self, inner, diag):
        self.inner, self.diag = inner, torch.tensor(diag, dtype=torch.float64)

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        for b in self.inner:
            aff = b["image_meta_dict"]["original_affine"].clone().double()
            for k in range(3):
                aff[:, k, k] = self.diag[k]
            b["image_meta_dict"]["original_affine"] = aff
            yield b


def test_train_one_epoch_with_affine_bias():
    from medicalsemseg_amd.data import SyntheticLoader
    from medicalsemseg_amd.engine.train import train_one_epoch
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay
    from medicalsemseg_amd.utils.arguments import get_args
    cfg = get_args(_ENGINE_ARGS.split())
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV)
    emb = model.encoder.layers[0].blocks[1].attn.rel_pos_bias_affine_emb
    emb0 = emb.detach().clone()
    opt = FlatAdamW(add_weight_decay(model, 1e-2), lr=2e-3, betas=(0.9, 0.95), eps=1e-6)
    loader = _SpacedLoader(SyntheticLoader(3, 2, 48, 1, 2, seed=1), [1.5, -0.8, 2.5])
    s = train_one_epoch(model, loader, opt, DiceCELoss(), torch.device(DEV), 0, torch.amp.GradScaler("cuda", enabled=False),
                        cfg)
    torch.cuda.synchronize()
    assert np.isfinite(s["train/loss"])
    assert emb.grad is not None and float(emb.grad.abs().max()) > 0
    assert not torch.equal(emb.detach(), emb0)


def test_sliding_window_with_affine_bias_equals_per_window_loop():
    """engine sliding-window inference (one affine row for a batch of windows) against the oracle's window loop driving the
    same model"""
    from medicalsemseg_amd.engine.utils import sliding_window_inference as sw_hip
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.utils.arguments import get_args
    from oracle.sliding_window import sliding_window_inference as sw_ref
    cfg = get_args(_ENGINE_ARGS.split())
    cfg.compute_dtype = "f32"
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV).eval()
    det_fill_(_AffineParams(model), "sw_aff")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 1, 56, 48, 64, generator=g)
    aff = torch.tensor([[0.8, -1.2, 2.5]])
    seen = []

    def loop_model(inp):
        win, _, a = inp
        seen.append(a.shape[0])
        return model((win.to(DEV), None, a.to(DEV))).float().cpu()

    with torch.no_grad():
        got = sw_hip(x.to(DEV), aff.to(DEV), (48, 48, 48), 2, model, overlap=0.5, mode="gaussian")
        want = sw_ref(x, aff, (48, 48, 48), 2, loop_model, overlap=0.5, mode="gaussian")
        plain = sw_hip(x.to(DEV), None, (48, 48, 48), 2, model, overlap=0.5, mode="gaussian")
    assert seen and all(n == 1 for n in seen)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=2e-4)
    assert float((got - plain).abs().max()) > 1e-3          # the spacing term is active


def test_run_training_driver_with_affine_bias(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "run_training.py"), "--synthetic", "--model", "nnFormerUNETR",
           "--rel_pos_bias_affine", "--output_dim", "2", "--vol_size", "48", "--patch_size", "2", "--hidden_dim", "32",
           "--depths", "2", "2", "--num_heads", "2", "4", "--window_size", "6", "3", "--qkv_bias", "--n_images_per_batch",
           "2", "--synthetic_steps", "2", "--epochs", "2", "--val_interval", "2", "--synthetic_val_size", "48",
           "--warmup_epochs", "1", "--output_dir", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(tmp_path / "log.txt")
