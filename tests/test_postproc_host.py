"""CPU-side checks around the post-processing steps: the scipy restatement the GPU tests compare with
(tests/postproc_ref.py) and the CLI flags."""
import numpy as np
import pytest

from tests.components_ref import keep_largest_ref
from tests.postproc_ref import fill_holes_dilation_ref, fill_holes_ref, postprocess_ref


def _noise(seed, shape=(12, 13, 20), p1=0.7):
    u = np.random.default_rng(seed).random(shape)
    lab = np.zeros(shape, np.uint8)
    lab[u < p1] = 1
    lab[u > 1.0 - (1.0 - p1) / 2] = 2
    return lab


@pytest.mark.parametrize("hole_conn", [6, 26])
def test_fill_holes_form_equals_monai_dilation_form(hole_conn):
    changed = 0
    for seed in range(4):
        lab = _noise(seed)
        lab[1:8, 1:8, 1:11] = 1
        lab[3:6, 3:6, 3:9] = 255                      # an ignore value enclosed by class 1: overwritten
        a, filled = fill_holes_ref(lab, 3, hole_conn)
        assert np.array_equal(a, fill_holes_dilation_ref(lab, 3, hole_conn))
        assert np.array_equal(postprocess_ref(lab, 3, fill_holes=True, hole_connectivity=hole_conn)[0], a)
        assert not (a == 255).any() and filled[1] >= 54
        changed += int((a != lab).sum())
    assert changed >= 4 * 54 + (20 if hole_conn == 6 else 0)      # at 6 the noise holds holes of its own


def test_fill_holes_leak_connectivity_and_sequential_rule():
    lab = np.zeros((7, 7, 7), np.uint8)
    lab[1:6, 1:6, 1:6] = 1
    lab[2:5, 2:5, 2:5] = 0                            # a 3^3 cavity
    lab[3, 3, 3] = 2
    out, stats = postprocess_ref(lab, 3, fill_holes=True, hole_connectivity=6)
    assert out.sum() == 125 and stats.tolist() == [[0] * 6, [-1, 0, 0, 0, 27, 125], [-1, 0, 0, 0, 0, 0]]
    lab[1, 1, 1] = 0                                  # the wall's corner voxel: touches the cavity's corner diagonally only
    assert postprocess_ref(lab, 3, fill_holes=True, hole_connectivity=6)[1][1, 4] == 27
    assert postprocess_ref(lab, 3, fill_holes=True, hole_connectivity=26)[1][1, 4] == 0
    lab = np.zeros((5, 5, 5), np.uint8)
    lab[:, :, :] = 1
    lab[2, 2, 0:3] = 0                                # a tunnel that opens onto a volume face: no hole
    assert np.array_equal(postprocess_ref(lab, 2, fill_holes=True)[0], lab)


@pytest.mark.parametrize("conn", [6, 26])
def test_keep_largest_only_equals_keep_largest_ref(conn):
    lab = _noise(7, p1=0.3)
    want, want_stats = keep_largest_ref(lab, 3, conn)
    out, stats = postprocess_ref(lab, 3, keep_largest=True, connectivity=conn)
    assert np.array_equal(out, want)
    assert stats[:, 0].tolist() == want_stats[:, 0].tolist() and stats[:, 3].tolist() == want_stats[:, 3].tolist()
    assert stats[:, 5].tolist() == want_stats[:, 1].tolist()       # without a fill step the class holds what was kept
    assert not stats[:, [1, 2, 4]].any() and want_stats[1, 0] > 1


def test_min_size_zero_and_one_are_no_ops_and_small_components_go():
    lab = _noise(8, p1=0.3)
    for n in (0, 1):
        out, stats = postprocess_ref(lab, 3, min_size=n)
        assert np.array_equal(out, lab) and stats[1:, 0].tolist() == [-1, -1] and not stats[:, 1:5].any()
        assert stats[:, 5].tolist() == [0, int((lab == 1).sum()), int((lab == 2).sum())]
    out, stats = postprocess_ref(lab, 3, min_size=3, connectivity=6)
    assert 0 < stats[1, 1] < stats[1, 0] and stats[1, 2] == int((lab == 1).sum()) - stats[1, 5]
    assert np.array_equal(out != lab, (lab > 0) & (out == 0))
    # a class whose largest component is below N ends up empty, and keep-largest then has nothing to remove
    lab = np.zeros((4, 4, 8), np.uint8)
    lab[0, 0, 0:3] = 1
    lab[2, 2, 0:2] = 1
    lab[1:3, 1:3, 4:8] = 2
    out, stats = postprocess_ref(lab, 3, min_size=4, keep_largest=True)
    assert stats.tolist() == [[0] * 6, [2, 2, 5, 0, 0, 0], [1, 0, 0, 0, 0, 16]] and not (out == 1).any()


def test_argument_defaults_and_choices():
    from medicalsemseg_amd.engine.test import post_enabled
    from medicalsemseg_amd.utils.arguments import get_args
    cfg = get_args([])
    assert cfg.post_min_size == 0 and cfg.post_fill_holes is False and cfg.post_hole_connectivity == 26
    assert not post_enabled(cfg)
    cfg = get_args("--post_min_size 64 --post_fill_holes --post_hole_connectivity 6".split())
    assert cfg.post_min_size == 64 and cfg.post_fill_holes is True and cfg.post_hole_connectivity == 6
    assert cfg.post_keep_largest is False and cfg.post_connectivity == 26 and post_enabled(cfg)
    for one in ("--post_min_size 2", "--post_fill_holes", "--post_keep_largest"):
        assert post_enabled(get_args(one.split()))
    assert not post_enabled(get_args("--post_min_size 1 --post_hole_connectivity 6".split()))
    with pytest.raises(SystemExit):
        get_args("--post_hole_connectivity 18".split())
