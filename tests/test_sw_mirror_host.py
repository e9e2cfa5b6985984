"""Host side of mirror test-time augmentation (--infer_mirror_axes): the mask helper, the flag, and self-checks of the CPU
restatement tests/sw_mirror_ref.py that the GPU tests (tests/test_gpu_sw_mirror.py) compare against."""
import pytest
import torch

from tests import sw_mirror_ref as mref
from tests.golden_util import SW_CASES, det_tensor, sw_predictor


def test_mirror_masks():
    from medicalsemseg_amd.engine.utils import mirror_masks
    assert mirror_masks(()) == (0,)
    assert mirror_masks((2,)) == (0, 4)
    assert mirror_masks((0, 2)) == (0, 1, 4, 5)
    assert mirror_masks((2, 0)) == (0, 1, 4, 5)
    assert mirror_masks((0, 1, 2)) == tuple(range(8))
    assert mirror_masks([1]) == (0, 2)
    assert mirror_masks(2) == (0, 4)
    assert mirror_masks(0) == (0, 1)
    for bad in ((3,), (1, 1), (-1,), 3, (0.0,), "01", None):
        with pytest.raises(ValueError, match="--infer_mirror_axes"):
            mirror_masks(bad)


def test_infer_mirror_axes_flag():
    from medicalsemseg_amd.engine.utils import mirror_masks
    from medicalsemseg_amd.utils.arguments import get_args
    cfg = get_args([])
    assert cfg.infer_mirror_axes == () and mirror_masks(cfg.infer_mirror_axes) == (0,)
    cfg = get_args("--infer_mirror_axes 0 1 2".split())
    assert cfg.infer_mirror_axes == (0, 1, 2) and mirror_masks(cfg.infer_mirror_axes) == tuple(range(8))
    cfg = get_args("--infer_mirror_axes 2".split())
    assert cfg.infer_mirror_axes == 2 and mirror_masks(cfg.infer_mirror_axes) == (0, 4)
    with pytest.raises(ValueError, match="--infer_mirror_axes"):
        mirror_masks(get_args("--infer_mirror_axes 1 3".split()).infer_mirror_axes)


@pytest.mark.parametrize("case", SW_CASES, ids=[c[0] for c in SW_CASES])
def test_ref_with_one_mask_is_the_oracle_loop(case):
    """padding, non-cubic ROI, the centers quirk at sw_batch_size 1, two volumes with a short last batch"""
    from oracle.sliding_window import sliding_window_inference
    tag, vol, roi, sb, ov, mode, cval = case
    x = det_tensor("sw_x_" + tag, vol)
    aff = det_tensor("sw_aff_" + tag, (vol[0], 3))
    want = sliding_window_inference(x, aff, roi, sb, sw_predictor, overlap=ov, mode=mode, cval=cval)
    got = mref.sliding_window_mirror_ref(x, aff, roi, sb, sw_predictor, overlap=ov, mode=mode, cval=cval)
    assert torch.equal(got, want)


def test_ref_with_eight_masks_on_a_flip_equivariant_predictor():
    """a pointwise predictor commutes with flips, so every mask contributes the logits the identity does and the weighted
    mean over 8 masks is the mean over 1; the two sums differ in length only: at overlap 0.5 at most 8 windows x 8 masks
    fp32 additions per voxel, 64 * 2^-24 * max|logit| absolute"""
    def pointwise(model_in):
        win = model_in[0]
        return torch.cat([win * 0.5 + 1.0, win.abs() - 2.0, win * win], dim=1)

    x = det_tensor("sw_mirror_eq", (1, 1, 20, 24, 28))
    kw = dict(overlap=0.5, mode="gaussian", cval=-0.75)
    one = mref.sliding_window_mirror_ref(x, None, (8, 8, 12), 3, pointwise, **kw)
    eight = mref.sliding_window_mirror_ref(x, None, (8, 8, 12), 3, pointwise, mirror_axes=(0, 1, 2), **kw)
    tol = 64 * 2.0 ** -24 * float(one.abs().max())
    err = float((eight - one).abs().max())
    print(f"max |8 masks - 1 mask| = {err:.3e}, bound {tol:.3e}")
    assert err <= tol


def test_ref_is_not_fooled_by_a_mirrored_weight():
    """the ROI (8, 8, 12) is even: its Gaussian map peaks at R // 2 and differs from its own mirror image, which is what lets
    the GPU comparison catch a weight indexed in window orientation"""
    from medicalsemseg_amd.engine.utils import importance_map
    imp = importance_map((8, 8, 12), "gaussian")
    for d in range(3):
        assert not torch.equal(imp, torch.flip(imp, [d]))
