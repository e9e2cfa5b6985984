"""GPU tests of TverskyLoss and DiceFocalLoss (the loss kinds of the fused passes in csrc/loss_sw.hip) against the float64
evaluation of tests/losses_ref.py: value and gradient of 3 * loss on NCDHW inputs, on channels-last 16-byte rows (the
vector-load path, as models/unet.py hands its logits over) and on the N > 8 atomic path; by-products, determinism, the
training / validation loops with the captured step, and the run_training.py switch.

Tolerances are those of tests/test_gpu_kernels.py::test_dice_ce: loss within 1e-5 * max(1, |ref|), fp32 gradients rtol 1e-4,
atol 1e-9; bf16 gradients to the bound of check() there (6e-3 of the reference's largest magnitude)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.losses_ref import dice_focal_loss, tversky_loss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ALPHA, BETA = 0.3, 0.7
KINDS = ["tversky", "dice_focal"]


def _crit(kind):
    from medicalsemseg_amd.losses import DiceFocalLoss, TverskyLoss
    return TverskyLoss(alpha=ALPHA, beta=BETA, smooth_nr=1e-5, smooth_dr=1e-5) if kind == "tversky" else DiceFocalLoss(
        smooth_nr=1e-5, smooth_dr=1e-5)


def _ref64(kind, logits, labels):
    """float64 loss and gradient of 3 * loss w.r.t. the logits"""
    x = logits.double().clone().requires_grad_(True)
    loss = tversky_loss(x, labels, ALPHA, BETA, 1e-5, 1e-5) if kind == "tversky" else dice_focal_loss(x, labels, 1e-5, 1e-5)
    (loss * 3.0).backward()
    return float(loss.detach()), x.grad


def _case(N, C, sp, seed=1):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, C, *sp, generator=g) * 2
    labels = torch.randint(0, C, (N, 1, *sp), generator=g)
    labels[1][labels[1] == C - 1] = 0   # a class absent from sample 1
    return logits, labels


def _check_fp32(kind, what, loss, grad, ref, gref):
    lerr = abs(float(loss) - ref) / max(1.0, abs(ref))
    d = (grad.double().cpu() - gref).abs()
    print(f"{kind} {what}: loss {float(loss):.8f} ref {ref:.8f} err {lerr:.2e}; grad max|d| {float(d.max()):.3e}, "
          f"worst |d| - (1e-4 |ref| + 1e-9) {float((d - (1e-4 * gref.abs() + 1e-9)).max()):.3e}, max|ref| {float(gref.abs().max()):.3e}")
    assert lerr < 1e-5
    np.testing.assert_allclose(grad.double().cpu().numpy(), gref.numpy(), rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,lab_dtype", [(3, torch.float32), (2, torch.int64), (14, torch.uint8)])
def test_value_and_gradient_ncdhw(kind, C, lab_dtype):
    """1680 voxels per sample: a ragged last trip of the 1024-voxel loop; CMAX 4 / 4 / 16 instantiations"""
    logits, labels = _case(2, C, (12, 10, 14))
    ref, gref = _ref64(kind, logits, labels)
    lg = logits.to(DEV).requires_grad_(True)
    loss = _crit(kind)(lg, labels.to(DEV).to(lab_dtype))
    (loss * 3.0).backward()
    _check_fp32(kind, f"C={C}", loss, lg.grad, ref, gref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,ld", [(torch.bfloat16, 8), (torch.float32, 4)])
def test_value_and_gradient_channels_last_rows(kind, dtype, ld):
    """logits as the [N, C, D, H, W] view of 16-byte channels-last rows (one vector load / store per voxel): the gradient
    comes back in the same rows, padding channels exactly zero, and the producer finds the rows through channels_last_grad"""
    from medicalsemseg_amd.losses import channels_last_grad
    C = 3
    logits, labels = _case(2, C, (12, 10, 14))
    rows = torch.full((2, 12, 10, 14, ld), 7.0)                      # the padding channels hold anything but zero
    rows[..., :C] = logits.permute(0, 2, 3, 4, 1)
    rows = rows.to(DEV, dtype).requires_grad_(True)
    view = rows[..., :C].permute(0, 4, 1, 2, 3)
    seen = []
    view.register_hook(seen.append)
    ref, gref = _ref64(kind, rows.detach()[..., :C].permute(0, 4, 1, 2, 3).float().cpu(), labels)   # on the rounded logits
    loss = _crit(kind)(view, labels.to(DEV).float())
    (loss * 3.0).backward()
    assert loss.dtype == torch.float32 and abs(float(loss) - ref) < 1e-5 * max(1.0, abs(ref)), (float(loss), ref)
    g = seen[0]
    base = channels_last_grad(g, ld, dtype)
    assert base is not None and tuple(base.shape) == (2, 12, 10, 14, ld) and base.dtype == dtype
    assert float(base[..., C:].float().abs().max()) == 0.0
    assert torch.equal(base[..., :C].permute(0, 4, 1, 2, 3), g) and torch.equal(rows.grad[..., :C], base[..., :C])
    if dtype == torch.float32:
        _check_fp32(kind, "rows fp32", loss, g, ref, gref)
    else:
        err = float((g.double().cpu() - gref).abs().max()) / float(gref.abs().max())
        print(f"{kind} rows bf16: loss {float(loss):.8f} ref {ref:.8f}; grad max err / max|ref| {err:.3e}")
        assert err < 6e-3


@pytest.mark.parametrize("kind", KINDS)
def test_value_and_gradient_atomic_path(kind):
    """N = 9 > 8: atomic partial sums and the separate finalize"""
    logits, labels = _case(9, 3, (4, 5, 6))
    ref, gref = _ref64(kind, logits, labels)
    lg = logits.to(DEV).requires_grad_(True)
    loss = _crit(kind)(lg, labels.to(DEV))
    (loss * 3.0).backward()
    _check_fp32(kind, "N=9", loss, lg.grad, ref, gref)


@pytest.mark.parametrize("kind", KINDS)
def test_by_products_and_determinism(kind):
    from medicalsemseg_amd.losses import DiceCELoss
    logits, labels = _case(2, 3, (12, 10, 14))
    lab = labels.to(DEV).float()
    dce = DiceCELoss()
    dce(logits.to(DEV), lab)
    crit = _crit(kind)
    runs = []
    for _ in range(2):
        lg = logits.to(DEV).requires_grad_(True)
        loss = crit(lg, lab)
        loss.backward()
        runs.append((loss.detach().clone(), lg.grad.clone()))
        assert crit.last["of"] == (lg.data_ptr(), tuple(lg.shape))
        assert torch.equal(crit.last["hard"], dce.last["hard"])            # the metric counts do not depend on the loss
        parts = crit.last["parts"]
        assert parts.shape == (3,) and torch.equal(parts[0], loss.detach()) and torch.equal(parts[0], parts[1] + parts[2])
        assert float(parts[1]) > 0 and (float(parts[2]) == 0.0 if kind == "tversky" else float(parts[2]) > 0)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    if kind == "dice_focal":
        assert torch.equal(crit.last["parts"][1], dce.last["parts"][1])    # the Dice term is DiceCELoss's, bit for bit


@pytest.mark.parametrize("kind", KINDS)
def test_engine_trains_with_the_captured_step_and_validates(kind, monkeypatch):
    """train_one_epoch on UNetSmall 32^3: the loss falls over two epochs, the step runs from the captured graph and the replay
    agrees with the eager step to the bounds of test_gpu_engine.py::test_train_epoch_graph_replay_equals_eager; run_validation
    (sliding window + the criterion on fp32 NCDHW logits) gives a finite loss"""
    from medicalsemseg_amd.data import SyntheticLoader
    from medicalsemseg_amd.engine.train import _GraphedFwdBwd, train_one_epoch
    from medicalsemseg_amd.engine.val import run_validation
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay
    from medicalsemseg_amd.utils.arguments import get_args
    cfg = get_args("--model UNetSmall --output_dim 2 --vol_size 32 --gradient_clipping 1.0 --batch_size_val 2".split())

    def run(eager):
        if eager:
            monkeypatch.setenv("MSSEG_NO_TRAIN_GRAPH", "1")
        else:
            monkeypatch.delenv("MSSEG_NO_TRAIN_GRAPH", raising=False)
        torch.manual_seed(0)
        model = build_model(cfg).to(DEV)
        opt = FlatAdamW(add_weight_decay(model, 1e-5), lr=2e-3, betas=(0.9, 0.95), eps=1e-6)
        scaler = torch.amp.GradScaler("cuda", enabled=False)
        crit = _crit(kind)
        stats = [train_one_epoch(model, SyntheticLoader(4, 2, 32, 1, 2, seed=1), opt, crit, torch.device(DEV), e, scaler,
                                 cfg)["train/loss"] for e in range(2)]
        assert any(g.criterion() is crit for g in _GraphedFwdBwd._cache.values()) == (not eager)
        return stats, opt.flat_param.clone(), model, crit

    (la, pa, _, _), (lb, pb, model, crit) = run(True), run(False)
    assert np.isfinite(lb).all() and lb[1] < lb[0] and la[1] < la[0]
    assert la == pytest.approx(lb, rel=2e-4)
    assert float((pa - pb).abs().mean()) < 2e-4 and float((pa - pb).abs().max()) < 2e-3 * 8
    v = run_validation(model, SyntheticLoader(1, 1, 48, 1, 2, seed=3, with_crop_info=False), crit, torch.device(DEV), 1, cfg)
    assert set(v) >= {"val/loss", "val/mDice"} and np.isfinite(v["val/loss"])


@pytest.mark.parametrize("flags", [["--loss_fn", "Tversky", "--tversky_alpha", "0.3", "--tversky_beta", "0.7"],
                                   ["--loss_fn", "DiceFocal"]], ids=["Tversky", "DiceFocal"])
def test_run_training_driver_loss_fn(tmp_path, flags):
    cmd = [sys.executable, os.path.join(ROOT, "run_training.py"), "--synthetic", "--model", "UNetSmall", "--output_dim", "2",
           "--vol_size", "32", "--n_images_per_batch", "2", "--synthetic_steps", "2", "--epochs", "2", "--val_interval", "2",
           "--synthetic_val_size", "48", "--warmup_epochs", "1", "--output_dir", str(tmp_path), "--save_ckpt_freq", "2", *flags]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(tmp_path / "checkpoint-1.pth") and os.path.exists(tmp_path / "log.txt")
