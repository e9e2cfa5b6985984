"""GPU tests of the sigmoid (region) forms of DiceCELoss, TverskyLoss and DiceFocalLoss (the REGIONS instantiations of the
fused passes in csrc/loss_sw.hip) against the float64 evaluation of tests/region_ref.py: value, loss triple, partial sums,
hard counts and the gradient of 3 * loss on NCDHW inputs, on channels-last 16-byte rows and on the N > 8 atomic path;
determinism; the hard counts of a partition against the softmax route; the training / validation loops.

Tolerances are those of tests/test_gpu_losses.py: loss within 1e-5 * max(1, |ref|), fp32 gradients rtol 1e-4, atol 1e-9, bf16
gradients within 6e-3 of the reference's largest magnitude.  The partial sums (fp32 sums of at most 210 terms per (n, c),
wave-tree order) are held to rtol 1e-5 + atol 1e-5; the hard counts are integers and must be exact."""
import numpy as np
import pytest
import torch

from tests.region_ref import BRAIN_TUMOUR, loss_and_grad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA, BETA = 0.3, 0.7
KINDS = ["dice_ce", "tversky", "dice_focal"]
# 16 regions over the labels 0..9 and 31: label 7 is in no region, label 31 in every other one, bit 40 % 32 = 8 is set in
# some masks, which label 40 must not pick up
MASKS16 = tuple((((0x9E3779B1 * (c + 1)) >> 7) & 0x37F | (1 << 8 if c % 3 == 0 else 0) | (1 << 31 if c % 2 else 0) | 1 << (c % 7))
                & ~(1 << 7) for c in range(16))


def _crit(kind, masks):
    from medicalsemseg_amd.losses import DiceCELoss, DiceFocalLoss, TverskyLoss
    if kind == "tversky":
        return TverskyLoss(alpha=ALPHA, beta=BETA, smooth_nr=1e-5, smooth_dr=1e-5, regions=masks)
    return (DiceCELoss if kind == "dice_ce" else DiceFocalLoss)(smooth_nr=1e-5, smooth_dr=1e-5, regions=masks)


def _kind_id(kind):
    from medicalsemseg_amd import hip
    return {"dice_ce": hip.LOSS_DICE_CE, "tversky": hip.LOSS_TVERSKY, "dice_focal": hip.LOSS_DICE_FOCAL}[kind]


def _ref(kind, logits, labels, masks):
    return loss_and_grad(kind, logits, labels, masks, scale=3.0, snr=1e-5, sdr=1e-5, alpha=ALPHA, beta=BETA)


def _case(N, C, sp, values, seed=1):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, C, *sp, generator=g) * 2
    labels = torch.tensor(values)[torch.randint(0, len(values), (N, 1, *sp), generator=g)]
    labels[1][labels[1] == values[-1]] = values[0]   # a label value absent from sample 1
    return logits, labels


def _check_fp32(what, loss, grad, ref, gref):
    lerr = abs(float(loss) - ref) / max(1.0, abs(ref))
    d = (grad.double().cpu() - gref).abs()
    print(f"{what}: loss {float(loss):.8f} ref {ref:.8f} err {lerr:.2e}; grad max|d| {float(d.max()):.3e}, "
          f"worst |d| - (1e-4 |ref| + 1e-9) {float((d - (1e-4 * gref.abs() + 1e-9)).max()):.3e}, max|ref| {float(gref.abs().max()):.3e}")
    assert lerr < 1e-5
    np.testing.assert_allclose(grad.double().cpu().numpy(), gref.numpy(), rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [3, 16])
def test_value_and_gradient_ncdhw(kind, C):
    """210 voxels per sample: the tail of the 4-voxel trip and of the block; CMAX 4 and 16.  C = 3: the BrainTumour table on
    uint8 labels 0..3.  C = 16: int64 labels with a value in no region (7), the value 31 and the value 40 (target 0)."""
    from medicalsemseg_amd import hip
    if C == 3:
        masks, (logits, labels), lab_dtype = BRAIN_TUMOUR[0], _case(2, 3, (5, 6, 7), [0, 1, 2, 3]), torch.uint8
    else:
        masks, (logits, labels), lab_dtype = MASKS16, _case(2, 16, (5, 6, 7), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 40]), torch.int64
        assert all(not (m >> 7) & 1 for m in masks) and any(m >> 31 for m in masks) and any((m >> 8) & 1 for m in masks)
    (ref, first, second), pref, href, gref = _ref(kind, logits, labels, masks)
    lab = labels.to(DEV).to(lab_dtype)
    lg = logits.to(DEV).requires_grad_(True)
    crit = _crit(kind, masks)
    loss = crit(lg, lab)
    (loss * 3.0).backward()
    _check_fp32(f"{kind} C={C}", loss, lg.grad, ref, gref)
    parts = crit.last["parts"].double().cpu()
    print(f"{kind} C={C}: triple {parts.tolist()} ref {(ref, first, second)}")
    for got, want in zip(parts.tolist(), (ref, first, second)):
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
    assert torch.equal(crit.last["hard"].double().cpu(), href)
    partial, hard, loss3 = hip.seg_loss_fwd(logits.to(DEV), lab, C, 1e-5, 1e-5, _kind_id(kind), ALPHA, BETA, regions=masks)
    print(f"{kind} C={C}: partial max|d| {float((partial.double().cpu() - pref).abs().max()):.3e}")
    np.testing.assert_allclose(partial.double().cpu().numpy(), pref.numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(hard.double().cpu(), href) and torch.equal(loss3[0], loss.detach())
    if kind == "tversky":
        assert float(partial[..., 3].abs().max()) == 0.0 and float(loss3[2]) == 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,ld,C", [(torch.bfloat16, 8, 3), (torch.float32, 4, 3), (torch.bfloat16, 8, 5)])
def test_value_and_gradient_channels_last_rows(kind, dtype, ld, C):
    """logits as the [N, C, D, H, W] view of 16-byte channels-last rows, 13440 voxels per sample (seven blocks' rows): the
    gradient comes back through channels_last_grad, padding channels exactly zero.  The reference runs on the logits as
    rounded to the tested dtype."""
    from medicalsemseg_amd.losses import channels_last_grad
    sp = (20, 24, 28)
    masks = BRAIN_TUMOUR[0] if C == 3 else (0b11110, 0b11100, 0b11000, 0b10000, 0b00110)
    logits, labels = _case(2, C, sp, list(range(C + 1)))
    rows = torch.full((2, *sp, ld), 7.0)                                # the padding channels hold anything but zero
    rows[..., :C] = logits.permute(0, 2, 3, 4, 1)
    rows = rows.to(DEV, dtype).requires_grad_(True)
    view = rows[..., :C].permute(0, 4, 1, 2, 3)
    seen = []
    view.register_hook(seen.append)
    (ref, _, _), _, href, gref = _ref(kind, rows.detach()[..., :C].permute(0, 4, 1, 2, 3).float().cpu(), labels, masks)
    crit = _crit(kind, masks)
    loss = crit(view, labels.to(DEV).to(torch.uint8))
    (loss * 3.0).backward()
    print(f"{kind} rows {dtype} ld={ld} C={C}: loss {float(loss):.8f} ref {ref:.8f}")
    assert loss.dtype == torch.float32 and abs(float(loss) - ref) < 1e-5 * max(1.0, abs(ref)), (float(loss), ref)
    assert torch.equal(crit.last["hard"].double().cpu(), href)
    g = seen[0]
    base = channels_last_grad(g, ld, dtype)
    assert base is not None and tuple(base.shape) == (2, *sp, ld) and base.dtype == dtype
    assert float(base[..., C:].float().abs().max()) == 0.0
    assert torch.equal(base[..., :C].permute(0, 4, 1, 2, 3), g) and torch.equal(rows.grad[..., :C], base[..., :C])
    if dtype == torch.float32:
        _check_fp32(f"{kind} rows fp32", loss, g, ref, gref)
    else:
        err = float((g.double().cpu() - gref).abs().max()) / float(gref.abs().max())
        print(f"{kind} rows bf16 C={C}: grad max err / max|ref| {err:.3e}")
        assert err < 6e-3


@pytest.mark.parametrize("kind", KINDS)
def test_value_and_gradient_atomic_path(kind):
    """N = 9 > 8: atomic partial sums and the separate finalize"""
    masks = BRAIN_TUMOUR[0]
    logits, labels = _case(9, 3, (4, 5, 6), [0, 1, 2, 3])
    (ref, first, second), _, href, gref = _ref(kind, logits, labels, masks)
    lg = logits.to(DEV).requires_grad_(True)
    crit = _crit(kind, masks)
    loss = crit(lg, labels.to(DEV))
    (loss * 3.0).backward()
    _check_fp32(f"{kind} N=9", loss, lg.grad, ref, gref)
    assert torch.equal(crit.last["hard"].double().cpu(), href)
    for got, want in zip(crit.last["parts"].double().cpu().tolist(), (ref, first, second)):
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want))


@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_give_the_same_bits(kind):
    from medicalsemseg_amd import hip
    masks = BRAIN_TUMOUR[0]
    logits, labels = _case(2, 3, (20, 24, 28), [0, 1, 2, 3])
    lab = labels.to(DEV).to(torch.uint8)
    crit = _crit(kind, masks)
    runs = []
    for _ in range(2):
        lg = logits.to(DEV).requires_grad_(True)
        loss = crit(lg, lab)
        loss.backward()
        partial, hard, loss3 = hip.seg_loss_fwd(lg.detach(), lab, 3, 1e-5, 1e-5, _kind_id(kind), ALPHA, BETA, regions=masks)
        assert crit.last["of"] == (lg.data_ptr(), tuple(lg.shape))
        assert torch.equal(hard, crit.last["hard"]) and torch.equal(loss3, crit.last["parts"])
        runs.append((loss.detach().clone(), partial.clone(), hard.clone(), lg.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_partition_counts_equal_the_one_hot_counts():
    """masks 1 << c over C = 4 labels, every voxel's largest logit positive and the others negative: the thresholded region
    outputs ARE the arg-max one-hot, so `hard` must equal what the softmax route (dice_metric's pass) counts"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.losses import dice_metric
    C, sp = 4, (5, 6, 7)
    g = torch.Generator().manual_seed(5)
    logits = -(torch.randn(2, C, *sp, generator=g).abs() + 0.1)
    win = torch.randint(0, C, (2, 1, *sp), generator=g)
    logits.scatter_(1, win, torch.randn(2, 1, *sp, generator=g).abs() + 0.1)
    labels = torch.randint(0, C, (2, 1, *sp), generator=g)
    lg, lab = logits.to(DEV), labels.to(DEV).to(torch.uint8)
    _, soft_hard = hip.seg_loss_partials(lg, lab, C, hip.LOSS_DICE_CE, want_hard=True)
    masks = tuple(1 << c for c in range(C))
    for kind in KINDS:
        _, hard, _ = hip.seg_loss_fwd(lg, lab, C, 1e-5, 1e-5, _kind_id(kind), ALPHA, BETA, regions=masks)
        assert torch.equal(hard, soft_hard)
        _, hard_atomic = hip.seg_loss_partials(lg, lab, C, _kind_id(kind), want_hard=True, regions=masks)
        assert torch.equal(hard_atomic, soft_hard)
    a, b = dice_metric(lg, lab, regions=masks), dice_metric(lg, lab)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float(soft_hard[..., 1].sum()) == 2 * 5 * 6 * 7


def test_entry_points_refuse_a_bad_channel_count():
    from medicalsemseg_amd import hip
    lg = torch.zeros(1, 17, 2, 2, 2, device=DEV)
    lab = torch.zeros(1, 1, 2, 2, 2, dtype=torch.uint8, device=DEV)
    rm = hip.region_masks((1,) * 16)
    p = torch.zeros(1, 17, 4, device=DEV)
    loss = torch.zeros(3, device=DEV)
    EINVAL = -1                                              # MSSEG_EINVAL of include/msseg.h
    for C in (0, 17):
        assert hip.lib().msseg_region_loss_partials(lg.data_ptr(), 0, hip.dt(lg), lab.data_ptr(), 2, p.data_ptr(), None, 1, 8, C,
                                                    0, rm, None) == EINVAL
        assert hip.lib().msseg_region_loss_finalize(p.data_ptr(), loss.data_ptr(), 1, 8, C, 1e-5, 1e-5, 0, 0.0, 0.0,
                                                    None) == EINVAL
        assert hip.lib().msseg_region_loss_bwd(lg.data_ptr(), 0, hip.dt(lg), lab.data_ptr(), 2, p.data_ptr(), None, lg.data_ptr(),
                                               0, 1, 8, C, 1e-5, 1e-5, 0, 0.0, 0.0, rm, None) == EINVAL
    with pytest.raises(ValueError, match="region"):
        hip.seg_loss_partials(lg[:, :3].contiguous(), lab, 3, 0, regions=(1, 2))


def test_engine_trains_with_the_captured_step_and_validates():
    """train_one_epoch on UNetSmall 32^3 with --output_dim 2 --label_regions 1,2=1 2=2 (labels 0..2): the step runs from the
    captured graph, the loss is finite and falls over two epochs; run_validation reports the per-region Dice meters and,
    with --post_keep_largest, ppDice"""
    from medicalsemseg_amd.data import SyntheticLoader
    from medicalsemseg_amd.engine.train import _GraphedFwdBwd, train_one_epoch
    from medicalsemseg_amd.engine.val import run_validation
    from medicalsemseg_amd.losses import build_criterion
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.optim import FlatAdamW, add_weight_decay
    from medicalsemseg_amd.utils.arguments import get_args, n_label_values
    cfg = get_args("--model UNetSmall --output_dim 2 --label_regions 1,2=1 2=2 --vol_size 32 --gradient_clipping 1.0 "
                   "--batch_size_val 2 --post_keep_largest".split())
    assert n_label_values(cfg) == 3
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV)
    opt = FlatAdamW(add_weight_decay(model, 1e-5), lr=2e-3, betas=(0.9, 0.95), eps=1e-6)
    scaler = torch.amp.GradScaler("cuda", enabled=False)
    crit = build_criterion(cfg)
    assert crit.regions == (0b110, 0b100)
    stats = [train_one_epoch(model, SyntheticLoader(4, 2, 32, 1, 3, seed=1), opt, crit, torch.device(DEV), e, scaler, cfg)
             for e in range(2)]
    assert any(g.criterion() is crit for g in _GraphedFwdBwd._cache.values())
    losses = [s["train/loss"] for s in stats]
    print("region training losses", losses)
    assert np.isfinite(losses).all() and losses[1] < losses[0]
    assert {"train/class0Dice", "train/class1Dice"} <= set(stats[1])
    v = run_validation(model, SyntheticLoader(1, 1, 48, 1, 3, seed=3, with_crop_info=False), crit, torch.device(DEV), 1, cfg)
    print("region validation", v)
    assert set(v) >= {"val/loss", "val/mDice", "val/class0Dice", "val/class1Dice", "val/ppDice"} and np.isfinite(v["val/loss"])
    assert "val/class2Dice" not in v and 0.0 <= v["val/ppDice"] <= 1.0
