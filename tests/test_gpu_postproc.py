"""msseg_postprocess_u8 (csrc/components.hip: small-component removal and keep-largest on one labelling, then hole filling
by labelling the complement of each class) against the scipy restatement tests/postproc_ref.py: the output map and all six
stats columns are compared exactly.  The kernel's tile is 8 x 8 x 32 voxels; the shapes straddle it in every axis and stay
under 96^3.  Then the engine entry points with the ``--post_*`` flags, driven by fixed logits (no trained model)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.components_ref import keep_largest_ref
from tests.postproc_ref import postprocess_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONNS = (6, 26)


def _run(lab: np.ndarray, n_classes: int, **kw):
    from medicalsemseg_amd import hip
    out, stats = hip.postprocess_u8(torch.from_numpy(lab).to(DEV), n_classes, return_stats=True, **kw)
    return out.cpu().numpy(), stats.cpu().numpy()


def _check(lab: np.ndarray, n_classes: int, **kw):
    """device result == restatement; returns (out, stats) of the restatement"""
    want, want_stats = postprocess_ref(lab, n_classes, **kw)
    got, got_stats = _run(lab, n_classes, **kw)
    assert got_stats.dtype == np.int32 and got_stats.shape == (n_classes, 6)
    assert got_stats.tolist() == want_stats.tolist(), (kw, got_stats.tolist(), want_stats.tolist())
    assert got.dtype == np.uint8 and np.array_equal(got, want), (kw, int((got != want).sum()))
    return want, want_stats


@functools.lru_cache(maxsize=None)
def _smoothed_noise():
    """arg max of three channels of smoothed noise (sigma 1): 531 components at connectivity 6.  Shared, never written to."""
    from scipy import ndimage
    noise = np.random.default_rng(5).standard_normal((3, 20, 27, 45))
    return np.argmax(ndimage.gaussian_filter(noise, 1.0), axis=0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _bernoulli():
    """class 1 at p = 0.8, the rest split evenly between 0 and 2.  Shared, never written to."""
    u = np.random.default_rng(1).random((20, 27, 45))
    lab = np.ones(u.shape, np.uint8)
    lab[u >= 0.8] = 0
    lab[u >= 0.9] = 2
    return lab


# ---- steps 1 and 2 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("n", [2, 8, 64])
def test_min_size_on_smoothed_noise(n, conn):
    _, stats = _check(_smoothed_noise(), 3, min_size=n, connectivity=conn)
    removed, before = int(stats[:, 1].sum()), int(stats[:, 0].sum())
    assert 1 <= removed < before, (removed, before)              # at least one component goes and at least one stays
    if conn == 6:
        assert (before, removed) == (531, {2: 299, 8: 464, 64: 525}[n])


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("n", [2, 8, 64])
def test_min_size_with_keep_largest(n, conn):
    lab = _smoothed_noise()
    want, stats = _check(lab, 3, min_size=n, keep_largest=True, connectivity=conn)
    assert np.array_equal(want, keep_largest_ref(lab, 3, conn)[0])      # the largest components here are above 64 voxels
    assert stats[1:, 1].min() >= 1 and (n > 2 or stats[1:, 3].min() >= 1)      # both steps remove voxels of both classes


@pytest.mark.parametrize("conn", CONNS)
def test_class_whose_largest_component_is_small_ends_up_empty(conn):
    lab = np.zeros((10, 12, 40), np.uint8)
    lab[1:3, 1:3, 30:34] = 1                                  # 16 voxels across the tile border x = 32: the largest of class 1
    lab[6:8, 10, 3:6] = 1                                     # 6 voxels
    lab[2:9, 2:10, 5:25] = 2
    lab[9, 11, 39] = 2
    for keep in (False, True):
        want, stats = _check(lab, 3, min_size=17, keep_largest=keep, connectivity=conn)
        assert not (want == 1).any() and stats[1].tolist() == [2, 2, 22, 0, 0, 0]
        assert stats[2].tolist() == [2, 1, 1, 0, 0, 7 * 8 * 20]


# ---- step 3 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hole_conn", CONNS)
def test_fill_on_bernoulli_noise(hole_conn):
    lab = _bernoulli()
    want, stats = _check(lab, 3, fill_holes=True, hole_connectivity=hole_conn)
    if hole_conn == 6:
        assert int((want != lab).sum()) >= 100 and int((want == 0).sum()) >= 100


def _hollow_box():
    """class 1 box with walls three voxels thick in 40 x 40 x 72; the cavity spans 5 x 5 x 3 tiles and holds one class 2
    voxel"""
    lab = np.zeros((40, 40, 72), np.uint8)
    lab[3:37, 3:37, 3:69] = 1
    lab[6:34, 6:34, 6:66] = 0
    lab[20, 21, 40] = 2
    return lab


@pytest.mark.parametrize("hole_conn", CONNS)
def test_fill_hollow_box_across_tiles(hole_conn):
    lab = _hollow_box()
    want, stats = _check(lab, 3, fill_holes=True, hole_connectivity=hole_conn)
    assert (want[3:37, 3:37, 3:69] == 1).all() and stats[1, 4] == 28 * 28 * 60 and stats[2].tolist() == [-1, 0, 0, 0, 0, 0]


def test_fill_diagonal_channel_leaks_at_26_only():
    lab = _hollow_box()
    for k in range(3):                                        # through the wall x = 3..5: each voxel touches the next at a
        lab[21 + k, 21 + k, 3 + k] = 0                        # corner only; the last one meets the cavity's (24, 24, 6)
    _, s6 = _check(lab, 3, fill_holes=True, hole_connectivity=6)
    _, s26 = _check(lab, 3, fill_holes=True, hole_connectivity=26)
    assert s6[1, 4] == 28 * 28 * 60 + 2 and s26[1, 4] == 0    # at 6 the two inner channel voxels are holes as well


@pytest.mark.parametrize("face", range(6))
def test_cavity_open_to_one_volume_face_is_not_filled(face):
    lab = np.ones((12, 13, 40), np.uint8)
    lab[4:8, 4:9, 10:36] = 0
    tunnel = [(slice(0, 4), 6, 20), (slice(8, 12), 6, 20), (5, slice(0, 4), 20), (5, slice(9, 13), 20),
              (5, 6, slice(0, 10)), (5, 6, slice(36, 40))][face]
    closed = _check(lab, 2, fill_holes=True)[1]
    assert closed[1, 4] == 4 * 5 * 26
    lab[tunnel] = 0
    for hole_conn in CONNS:
        want, stats = _check(lab, 2, fill_holes=True, hole_connectivity=hole_conn)
        assert np.array_equal(want, lab) and stats[1, 4] == 0


def test_cavity_reaching_the_volume_through_a_corner_voxel():
    lab = np.ones((10, 11, 36), np.uint8)
    lab[4:7, 4:7, 4:34] = 0
    for k in range(4):
        lab[k, k, k] = 0                                      # (0, 0, 0) is the volume's corner; (3, 3, 3) meets (4, 4, 4)
    _, s6 = _check(lab, 2, fill_holes=True, hole_connectivity=6)
    _, s26 = _check(lab, 2, fill_holes=True, hole_connectivity=26)
    assert s6[1, 4] == 3 * 3 * 30 + 3 and s26[1, 4] == 0


@pytest.mark.parametrize("hole_conn", CONNS)
def test_nested_shells_fill_in_class_order(hole_conn):
    lab = np.zeros((16, 16, 16), np.uint8)
    lab[1:15, 1:15, 1:15] = 1
    lab[3:13, 3:13, 3:13] = 2
    lab[5:11, 5:11, 5:11] = 1
    lab[7:9, 7:9, 7:9] = 0
    want, stats = _check(lab, 3, fill_holes=True, hole_connectivity=hole_conn)
    assert (want[1:15, 1:15, 1:15] == 1).all() and stats[1].tolist() == [-1, 0, 0, 0, 10 ** 3 - 6 ** 3 + 8, 14 ** 3]
    assert stats[2].tolist() == [-1, 0, 0, 0, 0, 0]           # class 1 took the shell of class 2 before its turn came


def _serpentine_cavity():
    """a one-voxel-wide path of class 0 inside a solid class 1 volume of 24 x 24 x 96 (3 x 3 x 3 tiles): rows along x at odd
    y joined at alternating ends, odd planes joined where the path arrives; no voxel of it on a face.  Returns (map, the
    path's length, a face voxel next to its last voxel)."""
    lab = np.ones((24, 24, 96), np.uint8)
    ys, zs = list(range(1, 23, 2)), list(range(1, 23, 2))
    x_at = 1
    for kz, z in enumerate(zs):
        order = ys if kz % 2 == 0 else ys[::-1]
        for ky, y in enumerate(order):
            lab[z, y, 1:95] = 0
            x_at = 94 if x_at == 1 else 1
            if ky + 1 < len(order):
                lab[z, (y + order[ky + 1]) // 2, x_at] = 0
        if kz + 1 < len(zs):
            lab[z + 1, order[-1], x_at] = 0
    return lab, int((lab == 0).sum()), (zs[-1], order[-1], 95 if x_at == 94 else 0)


@pytest.mark.parametrize("hole_conn", CONNS)
def test_serpentine_cavity_through_every_tile(hole_conn):
    lab, length, exit_voxel = _serpentine_cavity()
    for tz in range(3):
        for ty in range(3):
            for tx in range(3):
                assert (lab[8 * tz:8 * tz + 8, 8 * ty:8 * ty + 8, 32 * tx:32 * tx + 32] == 0).any()
    want, stats = _check(lab, 2, fill_holes=True, hole_connectivity=hole_conn)
    assert want.all() and stats[1].tolist() == [-1, 0, 0, 0, length, lab.size]
    lab[exit_voxel] = 0                                       # opened at the far end from the component's first voxel
    want, stats = _check(lab, 2, fill_holes=True, hole_connectivity=hole_conn)
    assert np.array_equal(want, lab) and stats[1, 4] == 0


# ---- all three, edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hole_conn", CONNS)
@pytest.mark.parametrize("conn", CONNS)
def test_all_three_steps(conn, hole_conn):
    for lab in (_smoothed_noise(), _bernoulli()):
        _check(lab, 3, min_size=8, keep_largest=True, connectivity=conn, fill_holes=True, hole_connectivity=hole_conn)
        _check(lab, 3, min_size=8, connectivity=conn, fill_holes=True, hole_connectivity=hole_conn)


ALL_ON = dict(min_size=3, keep_largest=True, fill_holes=True)


def test_tiny_uniform_and_odd_volumes():
    for value in (0, 1):
        _, stats = _check(np.full((1, 1, 1), value, np.uint8), 2, **ALL_ON)
        assert stats[1].tolist() == ([1, 1, 1, 0, 0, 0] if value else [0] * 6)
        for kw in (ALL_ON, dict(fill_holes=True), dict(min_size=3)):
            _check(np.full((9, 9, 33), value, np.uint8), 3, **kw)
    _, stats = _check(np.ones((9, 9, 33), np.uint8), 3, **ALL_ON)
    assert stats.tolist() == [[0] * 6, [1, 0, 0, 0, 0, 9 * 9 * 33], [0] * 6]
    lab = np.random.default_rng(3).integers(0, 3, (9, 9, 33)).astype(np.uint8)
    for conn in CONNS:
        _check(lab, 3, connectivity=conn, hole_connectivity=conn, **ALL_ON)


def test_values_beyond_the_classes():
    rng = np.random.default_rng(2)
    lab = rng.integers(0, 3, (17, 18, 67)).astype(np.uint8)
    lab[rng.random(lab.shape) < 0.2] = 255
    lab[5:12, 4:14, 30:36] = 255                              # a wall of 255 across a tile border
    for conn in CONNS:
        want, _ = _check(lab, 3, min_size=4, keep_largest=True, connectivity=conn)
        assert np.array_equal(want == 255, lab == 255)        # steps 1 and 2 copy them
    lab = np.zeros((17, 18, 67), np.uint8)
    lab[2:15, 2:16, 20:50] = 2
    lab[5:9, 5:9, 28:36] = 255                                # enclosed by class 2: overwritten
    lab[0:3, 0:3, 60:67] = 255                                # on the volume's faces: stays
    for hole_conn in CONNS:
        want, stats = _check(lab, 3, fill_holes=True, hole_connectivity=hole_conn)
        assert stats[2, 4] == 4 * 4 * 8 and int((want == 255).sum()) == 3 * 3 * 7


def test_in_place_repeatable_and_all_off_is_a_copy():
    from medicalsemseg_amd import hip
    lab = _smoothed_noise()
    t = torch.from_numpy(lab).to(DEV)
    kw = dict(min_size=8, keep_largest=True, connectivity=6, fill_holes=True, hole_connectivity=6)
    a, sa = hip.postprocess_u8(t, 3, return_stats=True, **kw)
    b, sb = hip.postprocess_u8(t, 3, return_stats=True, **kw)
    assert torch.equal(a, b) and torch.equal(sa, sb)                   # identical bytes from run to run
    assert torch.equal(t.cpu(), torch.from_numpy(lab))                 # the input is left alone out of place
    assert not torch.equal(a, t)
    for sub in (kw, dict(fill_holes=True, hole_connectivity=6), dict(min_size=8)):
        buf = t.clone()
        c = hip.postprocess_u8(buf, 3, out=buf, **sub)
        assert c is buf and torch.equal(buf, hip.postprocess_u8(t, 3, **sub))
    for n in (0, 1):
        out, stats = hip.postprocess_u8(t, 3, min_size=n, return_stats=True)
        assert out is not t and torch.equal(out, t)
        assert stats.cpu().tolist() == postprocess_ref(lab, 3, min_size=n)[1].tolist()
    buf = t.clone()
    assert hip.postprocess_u8(buf, 3, out=buf) is buf and torch.equal(buf, t)


def test_refusals():
    from medicalsemseg_amd import hip
    t = torch.zeros(8, 8, 40, dtype=torch.uint8, device=DEV)
    with pytest.raises(hip.MssegError, match="connectivity 18"):
        hip.postprocess_u8(t, 3, connectivity=18)
    with pytest.raises(hip.MssegError, match="hole connectivity 18"):
        hip.postprocess_u8(t, 3, hole_connectivity=18)
    with pytest.raises(hip.MssegError, match="min_size -1"):
        hip.postprocess_u8(t, 3, min_size=-1)
    with pytest.raises(hip.MssegError, match="1 classes"):
        hip.postprocess_u8(t, 1)
    with pytest.raises(hip.MssegError, match="65 classes"):
        hip.postprocess_u8(t, 65)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.postprocess_u8(t.cpu(), 3)
    with pytest.raises(AssertionError, match="contiguous"):
        hip.postprocess_u8(t.permute(2, 1, 0), 3)
    with pytest.raises(AssertionError, match="uint8"):
        hip.postprocess_u8(t.int(), 3)
    assert hip.postprocess_u8(t, 3, min_size=2, fill_holes=True).sum().item() == 0      # usable after the refusals


@pytest.mark.parametrize("conn", CONNS)
def test_keep_largest_alone_equals_keep_largest_u8(conn):
    from medicalsemseg_amd import hip
    t = torch.from_numpy(_smoothed_noise()).to(DEV)
    old, old_stats = hip.keep_largest_u8(t, 3, conn, return_stats=True)
    new, new_stats = hip.postprocess_u8(t, 3, keep_largest=True, connectivity=conn, return_stats=True)
    assert torch.equal(old, new)
    old_stats, new_stats = old_stats.cpu(), new_stats.cpu()
    assert new_stats[:, 0].tolist() == old_stats[:, 0].tolist() and min(old_stats[1:, 0].tolist()) > 1      # components
    assert new_stats[:, 3].tolist() == old_stats[:, 3].tolist()                                             # removed
    assert new_stats[:, 5].tolist() == old_stats[:, 1].tolist()                                             # kept
    assert not new_stats[:, [1, 2, 4]].any()


# ---- engine -----------------------------------------------------------------------------------------------------------
def _ball_with_specks_and_a_hole(shape=(24, 28, 40)):
    """(label: one ball of class 1; prediction: the ball with a 3^3 hole, a 27-voxel island that --post_min_size 8 leaves and
    two specks it removes)"""
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    label = (((z - 12) ** 2 + (y - 14) ** 2 + (x - 20) ** 2) <= 49).astype(np.uint8)
    pred = label.copy()
    pred[11:14, 13:16, 19:22] = 0
    pred[2:5, 2:5, 2:5] = 1
    pred[19:21, 24:26, 35] = 1
    pred[3, 24, 32:35] = 1
    return label, pred


def _batch(image, label, name):
    aff = torch.eye(4)[None]
    return {"image": image, "label": torch.from_numpy(label)[None, None].float(),
            "image_meta_dict": {"original_affine": aff, "affine": aff.clone(), "filename_or_obj": [name]},
            "image_transforms": []}


FLAGS = "--post_min_size 8 --post_fill_holes"


def _engine_case():
    label, pred = _ball_with_specks_and_a_hole()
    want, stats = postprocess_ref(pred, 2, min_size=8, fill_holes=True)
    assert stats[1].tolist()[:5] == [4, 2, 7, 0, 27] and not np.array_equal(want, label)
    logits = torch.from_numpy(np.stack([1.0 - pred, pred.astype(np.float64)]).astype(np.float32))[None].to(DEV) * 4.0
    return label, pred, want, logits


def test_eval_model_reports_post_processed_meters(tmp_path):
    from medicalsemseg_amd import metrics
    from medicalsemseg_amd.engine.test import eval_model
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.utils.arguments import get_args
    label, pred, want, logits = _engine_case()
    loader = [_batch(torch.zeros(1, 1, *label.shape), label, "vol0")]
    inferer = lambda inputs, network: logits.clone()   # noqa: E731
    base = "--model UNetSmall --output_dim 2 --vol_size 16"
    plain = eval_model(inferer, torch.nn.Identity(), loader, DiceCELoss(), torch.device(DEV), get_args(base.split()))
    cfg = get_args(f"{base} {FLAGS} --save_eval_output --output_dir {tmp_path}".split())
    r = eval_model(inferer, torch.nn.Identity(), loader, DiceCELoss(), torch.device(DEV), cfg)
    assert set(r) == set(plain) | {"eval/ppDice", "eval/ppHdorffDist"}
    for k in plain:                                         # the existing meters keep their values
        assert abs(r[k] - plain[k]) <= 1e-6 * abs(plain[k]), k
    labels = loader[0]["label"].to(DEV)
    want_map = torch.from_numpy(want).to(DEV)
    dice = metrics.dice_from_maps(want_map, labels[0], 2)[0][0]
    hd, _ = metrics.hausdorff_mean(metrics.hausdorff95(want_map[None], labels, 2))
    assert r["eval/ppDice"] == float(dice.mean()) and r["eval/mDice"] < r["eval/ppDice"] < 1.0
    assert r["eval/ppHdorffDist"] == hd
    assert np.array_equal(np.load(os.path.join(tmp_path, "pred_vol0.npy")), want)        # the saved map is the processed one


class _SignModel:
    """stands in for a network under the sliding window: class 1 wherever the window is positive"""

    def eval(self):
        return self

    def __call__(self, model_in):
        win = model_in[0].float()
        return torch.cat([torch.zeros_like(win[:, :1]), win[:, :1]], dim=1)


def test_test_model_saves_the_processed_map(tmp_path, capsys):
    from medicalsemseg_amd.engine.test import test_model
    from medicalsemseg_amd.utils.arguments import get_args
    _, pred, want, _ = _engine_case()
    image = torch.from_numpy(np.where(pred > 0, 1.0, -1.0).astype(np.float32))[None, None]
    cfg = get_args(f"--model UNetSmall --output_dim 2 --vol_size 16 --batch_size_val 2 --save_eval_output {FLAGS} "
                   f"--output_dir {tmp_path}".split())
    assert test_model(_SignModel(), [_batch(image, pred, "vol0")], torch.device(DEV), cfg) is None
    assert np.array_equal(np.load(os.path.join(tmp_path, "test_output", "Fold0", "pred", "vol0.npy")), want)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("post-processing, vol0")]
    assert len(line) == 1 and "2 below 8 voxels removed (7 voxels)" in line[0] and "27 filled" in line[0]


def test_run_validation_adds_pp_dice_only_with_a_post_flag():
    from medicalsemseg_amd import metrics
    from medicalsemseg_amd.engine.val import run_validation
    from medicalsemseg_amd.losses import DiceCELoss
    from medicalsemseg_amd.utils.arguments import get_args
    label, pred, want, logits = _engine_case()
    loader = [_batch(torch.zeros(1, 1, *label.shape), label, "vol0")]
    inferer = lambda **kw: logits.clone()   # noqa: E731
    base = "--model UNetSmall --output_dim 2 --vol_size 16"
    dev = torch.device(DEV)
    plain = run_validation(torch.nn.Identity(), loader, DiceCELoss(), dev, 0, get_args(base.split()), inferer=inferer)
    assert set(plain) == {"val/loss", "val/mDice", "val/class0Dice", "val/class1Dice"}
    r = run_validation(torch.nn.Identity(), loader, DiceCELoss(), dev, 0, get_args(f"{base} {FLAGS}".split()), inferer=inferer)
    assert set(r) == set(plain) | {"val/ppDice"}
    for k in plain:
        assert r[k] == plain[k], k
    dice = metrics.dice_from_maps(torch.from_numpy(want).to(DEV), loader[0]["label"].to(DEV)[0], 2)[0][0]
    assert r["val/ppDice"] == float(dice.mean()) > plain["val/mDice"]
