"""CPU-side checks around the keep-largest-component step: the scipy restatement the GPU tests compare with
(tests/components_ref.py), the CLI defaults and metrics.dice_from_maps."""
import numpy as np
import torch

from tests.components_ref import keep_largest_ref


def test_restatement_tie_keeps_the_component_that_starts_first():
    lab = np.zeros((4, 5, 12), np.uint8)
    lab[2, 3, 6:9] = 1          # three voxels, first voxel at flat index 2 * 60 + 3 * 12 + 6
    lab[0, 4, 1:4] = 1          # three voxels, earlier in raster order: kept
    lab[1, 0, 0:2] = 1          # two voxels
    lab[3, 0, 0] = 2
    for conn in (6, 26):
        out, stats = keep_largest_ref(lab, 3, conn)
        want = np.zeros_like(lab)
        want[0, 4, 1:4] = 1
        want[3, 0, 0] = 2
        assert np.array_equal(out, want)
        assert stats.tolist() == [[0, 0, -1, 0], [3, 3, 4 * 12 + 1, 5], [1, 1, 3 * 60, 0]]


def test_restatement_corner_contact_joins_only_at_26():
    lab = np.zeros((8, 8, 8), np.uint8)
    lab[1:3, 1:3, 1:3] = 1      # 8 voxels
    lab[3:6, 3:6, 3:6] = 1      # 27 voxels, meets the first cube at the corner (2,2,2)-(3,3,3) only
    out6, st6 = keep_largest_ref(lab, 2, 6)
    assert st6[1].tolist() == [2, 27, (3 * 8 + 3) * 8 + 3, 8] and out6.sum() == 27 and out6[1:3, 1:3, 1:3].sum() == 0
    out26, st26 = keep_largest_ref(lab, 2, 26)
    assert st26[1].tolist() == [1, 35, (1 * 8 + 1) * 8 + 1, 0] and np.array_equal(out26, lab)


def test_restatement_copies_ignore_values_and_reports_absent_classes():
    lab = np.zeros((3, 3, 6), np.uint8)
    lab[0, 0, 0:2] = 1
    lab[0, 0, 2] = 255          # next to class 1: joins nothing, bridges nothing
    lab[0, 0, 3] = 1
    out, stats = keep_largest_ref(lab, 3, 26)
    assert out[0, 0].tolist() == [1, 1, 255, 0, 0, 0]
    assert stats.tolist() == [[0, 0, -1, 0], [2, 2, 0, 1], [0, 0, -1, 0]]


def test_argument_defaults_and_choices():
    import pytest
    from medicalsemseg_amd.utils.arguments import get_args
    cfg = get_args([])
    assert cfg.post_keep_largest is False and cfg.post_connectivity == 26
    cfg = get_args("--post_keep_largest --post_connectivity 6".split())
    assert cfg.post_keep_largest is True and cfg.post_connectivity == 6
    with pytest.raises(SystemExit):
        get_args("--post_connectivity 18".split())


def test_dice_from_maps_against_direct_counts():
    from medicalsemseg_amd.metrics import dice_from_maps
    rng = np.random.default_rng(4)
    C = 4
    pred = rng.integers(0, C, (5, 6, 7)).astype(np.uint8)
    label = rng.integers(0, 3, (1, 5, 6, 7)).astype(np.float32)       # class 3 absent from the label: NaN
    scores, not_nans = dice_from_maps(torch.from_numpy(pred), torch.from_numpy(label), C)
    assert scores.shape == (1, C) and not_nans.shape == (1, C)
    lab = label[0].astype(np.int64)
    for c in range(C):
        p, t = pred == c, lab == c
        if t.sum() == 0:
            assert np.isnan(float(scores[0, c])) and float(not_nans[0, c]) == 0.0
        else:
            want = np.float32(2.0) * np.float32((p & t).sum()) / np.float32(p.sum() + t.sum())
            assert float(scores[0, c]) == float(want) and float(not_nans[0, c]) == 1.0
    same, _ = dice_from_maps(torch.from_numpy(pred), torch.from_numpy(pred), C)
    assert same.tolist() == [[1.0] * C]
