"""GPU tests of mirror test-time augmentation inside the sliding-window kernels (the flips table of
msseg_sw_gather_batch / msseg_sw_blend_batch, sliding_window_inference(..., mirror_axes=...), --infer_mirror_axes).  The kernels are compared
bit for bit with compositions of the un-mirrored kernels and torch.flip, the whole function with the CPU restatement
tests/sw_mirror_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sw_mirror_ref as mref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _gen(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _flip_rows(t, masks, first_spatial_dim):
    """row k of t (dim 0) flipped along the axes of masks[k]; first_spatial_dim counts inside a row"""
    return torch.stack([torch.flip(t[k], mref.flip_dims(int(m), first_spatial_dim)) for k, m in enumerate(masks)])


# ---------------------------------------------------------------------------------------------------------------------
# 1. gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["fp32_ncdhw", "bf16_cl8"])
@pytest.mark.parametrize("roi", [(8, 8, 12), (7, 8, 11)])
def test_gather_mirror_is_flip_of_plain_gather(roi, layout):
    """eight rows, one per mask; a start hanging over the high edge; a shallow volume padded on both sides along D"""
    from medicalsemseg_amd import hip
    masks = list(range(8))
    fl = torch.tensor(masks, dtype=torch.int32, device=DEV)
    cases = [(_gen(1, 2, 20, 24, 28, seed=1), [(0, 0, 0), (4, 8, 6), (14, 20, 20), (12, 16, 16), (14, 20, 20), (3, 1, 2),
                                                (14, 20, 20), (13, 16, 17)]),
             (_gen(1, 2, 6, 24, 28, seed=2), [(-1, 3 * k, 2 * k) for k in range(8)]),
             (_gen(1, 2, roi[0] - 2, 24, 28, seed=3), [(-1, 20 - 2 * k, 20 - k) for k in range(8)])]
    for vol, starts in cases:
        table = torch.tensor([(0,) + s for s in starts], dtype=torch.int32, device=DEV)
        if layout == "fp32_ncdhw":
            new = lambda: torch.zeros(8, 2, *roi, device=DEV)   # noqa: E731
            kw, first = {}, 1
        else:
            new = lambda: torch.zeros(8, *roi, 8, dtype=torch.bfloat16, device=DEV)   # noqa: E731
            kw, first = {"channels_last_ld": 8}, 0
        plain = hip.sw_gather_batch(vol.to(DEV), new(), table, 8, cval=-3.0, **kw)
        got = hip.sw_gather_batch(vol.to(DEV), new(), table, 8, cval=-3.0, flips=fl, **kw)
        assert bool((plain == -3.0).any()) and bool((plain != -3.0).any())
        assert torch.equal(got, _flip_rows(plain, masks, first)), (roi, layout, tuple(vol.shape))
        # no mask on any row: the plain launch, through a zero table and through the null pointer of the C entry point
        zero = hip.sw_gather_batch(vol.to(DEV), new(), table, 8, cval=-3.0, flips=torch.zeros_like(fl), **kw)
        assert torch.equal(zero, plain)
        null = new()
        rc = hip.lib().msseg_sw_gather_batch(vol.to(DEV).data_ptr(), vol.stride(0), null.data_ptr(),
                                             kw.get("channels_last_ld", 0), hip.dt(null), table.data_ptr(), None, 8, 2,
                                             *vol.shape[2:], *roi, -3.0, None)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(null, plain)


# ---------------------------------------------------------------------------------------------------------------------
# 2. blend
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["fp32_ncdhw", "bf16_cl8"])
def test_blend_mirror_is_plain_blend_of_flipped_logits(layout):
    """the setting of test_sw_gather_blend with a start repeated under three masks; `imp` is positive and not symmetric, so
    a weight read at the mirrored index fails"""
    from medicalsemseg_amd import hip
    imp = _gen(8, 8, 12, seed=2).abs() + 0.1
    starts = [(0, 0, 0), (4, 8, 6), (4, 8, 6), (12, 16, 16), (4, 8, 6)]
    masks = [0, 5, 2, 7, 1]
    wins = torch.stack([_gen(3, 8, 8, 12, seed=10 + i) for i in range(5)])
    if layout == "bf16_cl8":
        wins = wins.bfloat16()
    # CPU loop: the un-mirrored logits, the weight in volume orientation
    oref, cref = torch.zeros(3, 20, 24, 28), torch.zeros(20, 24, 28)
    for w, st, m in zip(wins, starts, masks):
        sl = (slice(None), slice(st[0], st[0] + 8), slice(st[1], st[1] + 8), slice(st[2], st[2] + 12))
        oref[sl] += imp * torch.flip(w.float(), mref.flip_dims(m, 1))
        cref[sl[1:]] += imp
    table = torch.tensor([(0,) + st for st in starts] + [(-1, 0, 0, 0)], dtype=torch.int32, device=DEV)
    flips = torch.tensor(masks + [0], dtype=torch.int32, device=DEV)
    wd = torch.cat([wins, torch.zeros_like(wins[:1])])                         # the unused slot's window is never read
    unflipped = torch.cat([_flip_rows(wins, masks, 1), torch.zeros_like(wins[:1])])
    kw = {}
    if layout == "bf16_cl8":                                                   # 16-byte logits rows: the vector load
        def cl8(t):
            out = torch.zeros(t.shape[0], 8, 8, 12, 8, dtype=torch.bfloat16)
            out[..., :3] = t.permute(0, 2, 3, 4, 1)
            return out
        wd, unflipped, kw = cl8(wd), cl8(unflipped), {"channels_last_ld": 8}
    wd, unflipped, impd = wd.to(DEV), unflipped.to(DEV), imp.to(DEV)
    new = lambda: (torch.zeros(1, 3, 20, 24, 28, device=DEV), torch.zeros(1, 20, 24, 28, device=DEV))   # noqa: E731
    # the un-mirrored kernel fed the flipped logits, one row per launch in table order
    oseq, cseq = new()
    for k in range(5):
        hip.sw_blend_batch(unflipped[k:k + 1], impd, oseq, cseq, table[k:k + 1], 1, **kw)
    assert torch.equal(oseq[0].cpu(), oref) and torch.equal(cseq[0].cpu(), cref)
    # one launch with the unused last slot; two launches split in the middle of the repeated start
    for launches in ([(0, 6)], [(0, 2), (2, 4)]):
        out, cnt = new()
        for first, n in launches:
            hip.sw_blend_batch(wd[first:first + n], impd, out, cnt, table[first:first + n], n,
                               flips=flips[first:first + n], **kw)
        assert torch.equal(cnt, cseq), f"cnt max diff {float((cnt - cseq).abs().max())}"
        assert torch.equal(out, oseq), f"out max diff {float((out - oseq).abs().max())}"
    # no mask: the plain launch
    a, b = new(), new()
    hip.sw_blend_batch(wd, impd, *a, table, 6, **kw)
    hip.sw_blend_batch(wd, impd, *b, table, 6, flips=torch.zeros_like(flips), **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. end to end, tuple path
# ---------------------------------------------------------------------------------------------------------------------
_ROI = (16, 16, 24)


def _ramp_predictor():
    """position-sensitive and not flip-equivariant: seg[c] = win[:, 0] * ramp_c, one IEEE multiply per logit"""
    z = torch.arange(_ROI[0], dtype=torch.float32).view(-1, 1, 1)
    y = torch.arange(_ROI[1], dtype=torch.float32).view(1, -1, 1)
    x = torch.arange(_ROI[2], dtype=torch.float32).view(1, 1, -1)
    ramps = torch.stack([(0.25 + 0.125 * z + 0.0625 * x).expand(_ROI), (1.5 - 0.1875 * y + 0.03125 * z).expand(_ROI),
                         (0.5 + 0.0625 * z - 0.125 * y + 0.09375 * x).expand(_ROI)]).contiguous()
    calls = []

    def predictor(model_in):
        win, centers, _ = model_in
        calls.append((tuple(win.shape), centers.detach().cpu().clone()))
        return win[:, 0:1].float() * ramps.to(win.device)[None]

    return predictor, calls


_E2E = {"full": ((1, 1, 40, 36, 44), 0.0), "pad": ((1, 1, 12, 36, 44), 0.5)}
_ref_cache = {}


def _e2e_ref(case, axes):
    """computed once per (case, axes); read-only afterwards"""
    if (case, axes) not in _ref_cache:
        shape, cval = _E2E[case]
        pred, calls = _ramp_predictor()
        _ref_cache[case, axes] = (mref.sliding_window_mirror_ref(_gen(*shape, seed=21), None, _ROI, 3, pred, overlap=0.5,
                                                                 mode="gaussian", cval=cval, mirror_axes=axes), calls)
    return _ref_cache[case, axes]


@pytest.mark.parametrize("case,axes", [("full", ()), ("full", (1,)), ("full", (0, 2)), ("full", (0, 1, 2)),
                                       ("pad", (0, 1, 2))])
def test_sliding_window_mirror_matches_cpu_restatement(case, axes):
    """sw_batch_size 3 divides no mask count: batches straddle windows and the last one is short"""
    from medicalsemseg_amd.engine.utils import sliding_window_inference
    shape, cval = _E2E[case]
    x = _gen(*shape, seed=21)
    want, ref_calls = _e2e_ref(case, axes)
    pred, calls = _ramp_predictor()
    got = sliding_window_inference(x.to(DEV), None, _ROI, 3, pred, overlap=0.5, mode="gaussian", cval=cval,
                                   mirror_axes=axes)
    assert got.shape == want.shape == (shape[0], 3) + shape[2:]
    diff = float((got.cpu() - want).abs().max())
    print(f"{case} {axes}: max abs diff {diff:.3e} over {len(calls)} predictor calls")
    assert torch.equal(got.cpu(), want)
    # the predictor saw the same batches with the windows' own centers
    assert len(calls) == len(ref_calls)
    for (s0, c0), (s1, c1) in zip(calls, ref_calls):
        assert s0 == s1 and torch.equal(c0, c1)
    if axes == ():
        plain = sliding_window_inference(x.to(DEV), None, _ROI, 3, pred, overlap=0.5, mode="gaussian", cval=cval)
        assert torch.equal(plain, got)


def test_sliding_window_mirror_rejects_bad_axes():
    from medicalsemseg_amd.engine.utils import sliding_window_inference
    pred, _ = _ramp_predictor()
    with pytest.raises(ValueError, match="--infer_mirror_axes"):
        sliding_window_inference(torch.zeros(1, 1, 16, 16, 24, device=DEV), None, _ROI, 3, pred, mirror_axes=(0, 3))


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end, graph path
# ---------------------------------------------------------------------------------------------------------------------
def _composition(net, x, roi, nb, axes):
    """sliding_window_inference on the captured-graph path, restated with the UN-mirrored kernels: plain gather into a
    channels-last batch, torch.flip per row by its mask, eager net.infer_cl, flip back, plain blend, normalise -- in the same
    batch grouping"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.engine import utils as U
    size = tuple(x.shape[2:])
    starts = U.window_starts(size, roi, U.get_scan_interval(size, roi, 3, 0.5))
    masks = U.mirror_masks(axes)
    rows = [(st, m) for st in starts for m in masks]
    imp = U.importance_map(roi, "gaussian", 0.125, x.device)
    out = torch.zeros(1, net.out_channels, *size, device=x.device)
    cnt = torch.zeros(1, *size, device=x.device)
    for g0 in range(0, len(rows), nb):
        batch = rows[g0:g0 + nb]
        table = torch.tensor([(0,) + st for st, _ in batch] + [(-1, 0, 0, 0)] * (nb - len(batch)), dtype=torch.int32,
                             device=x.device)
        bm = [m for _, m in batch] + [0] * (nb - len(batch))
        win = torch.zeros(nb, *roi, 1, dtype=net.compute_dtype, device=x.device)
        hip.sw_gather_batch(x, win, table, nb, 0.0, channels_last_ld=1)
        seg = net.infer_cl(_flip_rows(win, bm, 0).contiguous())
        seg = _flip_rows(seg, bm, 0).contiguous()
        hip.sw_blend_batch(seg, imp, out, cnt, table, nb, channels_last_ld=seg.shape[-1])
    hip.sw_normalize(out[0], cnt[0])
    return out


def test_sliding_window_mirror_graph_path_matches_unmirrored_composition():
    """UNetSmall in bf16 on the replayed-graph path, 48^3 / roi 32^3 / 4 rows per replay / all 8 masks, against the
    composition of the un-mirrored kernels with torch.flip.  The one-mask composition is compared with the plain call first:
    whatever eager and replayed `infer_cl` differ by there belongs to the parent, and the mirrored comparison then allows
    twice that; where they agree bit for bit (the expectation) the mirrored result must too."""
    from medicalsemseg_amd.engine.utils import sliding_window_inference
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.utils.arguments import get_args
    cfg = get_args("--model UNetSmall --compute_dtype bf16 --in_chans 1 --output_dim 3 --vol_size 32".split())
    torch.manual_seed(3)
    net = build_model(cfg).to(DEV).eval()
    assert net.graph_safe and hasattr(net, "infer_cl")
    x = _gen(1, 1, 48, 48, 48, seed=31).to(DEV)
    roi = (32, 32, 32)
    with torch.no_grad():
        plain = sliding_window_inference(x, None, roi, 4, net, overlap=0.5, mode="gaussian")
        base = float((plain - _composition(net, x, roi, 4, ())).abs().max())
        got = sliding_window_inference(x, None, roi, 4, net, overlap=0.5, mode="gaussian", mirror_axes=(0, 1, 2))
        want = _composition(net, x, roi, 4, (0, 1, 2))
    diff = float((got - want).abs().max())
    print(f"one mask: replayed vs eager composition max abs diff {base:.3e}; eight masks: {diff:.3e}")
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, plain)
    if base == 0.0:
        assert torch.equal(got, want)
    else:
        assert diff <= 2.0 * base


# ---------------------------------------------------------------------------------------------------------------------
# 5. drivers
# ---------------------------------------------------------------------------------------------------------------------
def test_run_test_driver_and_eval_model_with_mirror_axes(tmp_path):
    from medicalsemseg_amd.data import SyntheticLoader
    from medicalsemseg_amd.engine.test import eval_model
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.utils.arguments import get_args
    base = ["--synthetic", "--model", "UNetSmall", "--output_dim", "2", "--vol_size", "32", "--synthetic_val_size", "48",
            "--batch_size_val", "2", "--infer_mirror_axes", "0", "1", "2"]
    cfg = get_args(base)
    torch.manual_seed(0)
    net = build_model(cfg)
    ck = str(tmp_path / "tiny.pth")
    torch.save({"model": net.state_dict(), "epoch": 0}, ck)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_test.py"), *base, "--resume", ck, "--synthetic_steps", "1",
                        "--save_eval_output", "--output_dir", str(tmp_path)], capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    pred = np.load(tmp_path / "test_output" / "Fold0" / "pred" / "synthetic_0_0.npy")
    assert pred.dtype == np.uint8 and pred.shape == (48, 48, 48)
    # eval_model, built-in inferer branch: finite meters with the flag, and not the meters of the un-mirrored call
    net = net.to(DEV).eval()
    loader = lambda: SyntheticLoader(1, 1, (32, 32, 48), 1, 2, seed=5, with_crop_info=False)   # noqa: E731
    ev = eval_model(None, net, loader(), DiceCELoss(), torch.device(DEV), cfg)
    assert set(ev) >= {"eval/loss", "eval/mDice"} and all(np.isfinite(v) for v in ev.values()), ev
    ev0 = eval_model(None, net, loader(), DiceCELoss(), torch.device(DEV), get_args(base[:-4]))
    assert ev0["eval/loss"] != ev["eval/loss"]
