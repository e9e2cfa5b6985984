"""Host side of the scorer (no GPU): known answers for the scipy restatement of the surface metrics
(tests/surface_ref.py), run_score.py's matching and refusals on tiny NIfTI files, run_predict.py's fold resolution."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from medicalsemseg_amd import data_files as df
from medicalsemseg_amd.utils.nifti import load_nifti, read_nifti_header, save_nifti
from tests import surface_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACING = (0.75, 1.5, 3.0)


def _slab(z, shape=(20, 9, 8)):
    m = np.zeros(shape, np.uint8)
    m[:, :, z] = 1
    return m


@pytest.mark.parametrize("k", [1, 2, 4])
def test_parallel_slabs_along_the_3mm_axis(k):
    """two one-voxel-thick slabs k voxels apart along the 3.0 mm axis: every surface voxel is 3k mm from the other slab"""
    pred, label = _slab(1), _slab(1 + k)
    below = sr.surface_metrics_ref(pred, label, 2, SPACING, np.nextafter(3.0 * k, 0.0))
    at = sr.surface_metrics_ref(pred, label, 2, SPACING, 3.0 * k)
    assert at["hd_mm"][1] == 3.0 * k and at["assd_mm"][1] == 3.0 * k
    assert below["nsd"][1] == 0.0 and at["nsd"][1] == 1.0                   # the comparison is <=
    assert below["hd_mm"][1] == at["hd_mm"][1]
    # the other axes take their own spacing: the same slabs along axis 0 are 0.75 k mm apart
    p0, l0 = np.moveaxis(pred, 2, 0), np.moveaxis(label, 2, 0)
    assert sr.surface_metrics_ref(p0, l0, 2, SPACING, 1.0)["hd_mm"][1] == 0.75 * k


def test_identical_maps_score_zero_zero_one():
    rng = np.random.default_rng(0)
    m = (rng.random((9, 10, 11)) < 0.3).astype(np.uint8) * 2
    got = sr.surface_metrics_ref(m, m.copy(), 3, SPACING, 1.0)
    for c in (0, 2):
        assert (got["hd_mm"][c], got["assd_mm"][c], got["nsd"][c]) == (0.0, 0.0, 1.0)
    assert all(np.isnan(got[k][1]) for k in got)                            # class 1: in neither map


def test_missing_class_conventions():
    label = np.zeros((6, 7, 8), np.uint8)
    label[2:4, 2:5, 3:6] = 1
    pred = label.copy()
    pred[pred == 1] = 2                                                     # class 1: label only; class 2: prediction only
    got = sr.surface_metrics_ref(pred, label, 4, SPACING, [1.0, 2.0, 3.0, 4.0])
    for c in (1, 2):
        assert got["hd_mm"][c] == np.inf and got["assd_mm"][c] == np.inf and got["nsd"][c] == 0.0
    assert all(np.isnan(got[k][3]) for k in got)                            # class 3: in neither map
    assert got["hd_mm"][0] == 0.0 and got["nsd"][0] == 1.0                  # the background is the same in both


def test_per_class_tolerances_are_applied_per_class():
    pred, label = _slab(1), _slab(3)
    got = sr.surface_metrics_ref(pred, label, 2, SPACING, [0.0, 6.0])
    assert got["nsd"][1] == 1.0
    assert sr.surface_metrics_ref(pred, label, 2, SPACING, [6.0, 5.9])["nsd"][1] == 0.0


# ---- run_score.py: matching and refusals, before any device is touched ----------------------------------------------------
def _task(tmp_path, **kw):
    rng = np.random.default_rng(1)
    labels = {f"{i:03d}": rng.integers(0, 3, (6, 7, 5)).astype(np.uint8) for i in range(3)}
    preds = {k: v.copy() for k, v in labels.items()}
    return labels, preds, sr.write_score_task(tmp_path, labels, preds, **kw)


def test_score_matches_predictions_to_labelled_cases_by_output_name(tmp_path):
    import run_score
    _, _, (data_path, task, pdir) = _task(tmp_path)
    js = df.datalist_path(data_path, task, "dataset.json")
    pairs = run_score.match_predictions(pdir, js)
    assert [p[0] for p in pairs] == ["000.nii.gz", "001.nii.gz", "002.nii.gz"]
    for name, pred_path, label_path in pairs:
        assert pred_path == os.path.join(pdir, name) and label_path == os.path.join(data_path, task, "labelsTr", name)
        spacing = run_score.check_pair(name, pred_path, label_path)
        assert np.allclose(spacing, (0.8, 0.8, 5.0), rtol=1e-6, atol=0)    # the sform is float32
    shape, aff = read_nifti_header(pairs[0][1])
    arr, aff2 = load_nifti(pairs[0][1])
    assert shape == arr.shape == (6, 7, 5) and np.array_equal(aff, aff2)


def test_score_refuses_a_prediction_without_a_labelled_partner(tmp_path):
    import run_score
    labels, _, (data_path, task, pdir) = _task(tmp_path)
    save_nifti(os.path.join(pdir, "t0.nii.gz"), labels["000"], sr.SCORE_AFFINE)   # the name of the unlabelled test case
    with pytest.raises(SystemExit, match="t0.nii.gz"):
        run_score.match_predictions(pdir, df.datalist_path(data_path, task, "dataset.json"))


def test_score_refuses_another_shape_and_another_affine(tmp_path):
    import run_score
    labels, _, (data_path, task, pdir) = _task(tmp_path)
    pairs = run_score.match_predictions(pdir, df.datalist_path(data_path, task, "dataset.json"))
    save_nifti(pairs[0][1], labels["000"][:, :6], sr.SCORE_AFFINE)
    with pytest.raises(SystemExit, match=r"000.nii.gz: shape \(6, 6, 5\)"):
        run_score.check_pair(*pairs[0])
    moved = sr.SCORE_AFFINE.copy()
    moved[1, 3] += 0.01                                                     # ten times the limit
    save_nifti(pairs[1][1], labels["001"], moved)
    with pytest.raises(SystemExit, match="001.nii.gz: affine differs"):
        run_score.check_pair(*pairs[1])
    scaled = sr.SCORE_AFFINE.copy()
    scaled[2, 2] = 2.5                                                      # same shape, another spacing
    save_nifti(pairs[2][1], labels["002"], scaled)
    with pytest.raises(SystemExit, match="002.nii.gz: affine differs"):
        run_score.check_pair(*pairs[2])


def test_score_script_refuses_before_it_asks_for_a_device(tmp_path):
    """the whole script on a folder with one wrong-grid map: the refusal names the file, whether or not a GPU is present"""
    labels, _, (data_path, task, pdir) = _task(tmp_path)
    moved = sr.SCORE_AFFINE.copy()
    moved[0, 3] -= 1.0
    save_nifti(os.path.join(pdir, "002.nii.gz"), labels["002"], moved)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_score.py"), "--pred_folder", pdir, "--data_path", data_path,
                        "--task", task, "--n_classes", "3"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "002.nii.gz: affine differs" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(os.path.join(pdir, "scores.json"))


def test_score_summary_means_finite_values_and_counts_misses():
    import run_score
    cases = {"a": {"dice": [1.0, 0.5], "hd_mm": [0.0, 2.0], "assd_mm": [0.0, 1.0], "nsd": [1.0, 0.5]},
             "b": {"dice": [1.0, 0.0], "hd_mm": [0.0, float("inf")], "assd_mm": [0.0, float("inf")], "nsd": [1.0, 0.0]},
             "c": {"dice": [1.0, float("nan")], "hd_mm": [0.0, 4.0], "assd_mm": [0.0, 3.0], "nsd": [1.0, 1.0]}}
    s = run_score.summarise(cases, 2)
    fg = s["foreground"]
    assert s["per_class"][1] == dict(fg, **{"class": 1})
    assert fg["n_cases"] == 3 and fg["n_missed"] == 1 and s["per_class"][0]["n_missed"] == 0
    assert fg["dice"] == 0.25 and fg["hd_mm"] == 3.0 and fg["assd_mm"] == 2.0 and fg["nsd"] == 0.5
    json.dumps(s)


# ---- run_predict.py: which cases "--test_section validation" means ----------------------------------------------------------
def test_predict_validation_section_falls_back_to_the_fold_split(tmp_path):
    import run_predict
    items = [{"image": f"./imagesTr/img{i}.nii.gz", "label": f"./labelsTr/{i}.nii.gz"} for i in range(11)]
    p = tmp_path / "dataset.json"
    p.write_text(json.dumps({"training": items, "test": ["./imagesTs/imgt.nii.gz"]}))
    train = df.load_datalist(str(p), "training")
    seen = []
    for fold in range(5):
        got = run_predict.section_files(str(p), "validation", 13, 5, fold)
        assert got == df.cv_split(train, 13, 5, fold)[1] and got
        seen += [g["image"] for g in got]
    assert sorted(seen) == sorted(t["image"] for t in train)               # the folds' held-out parts tile the list
    assert run_predict.section_files(str(p), "test", 13, 5, 0) == df.load_datalist(str(p), "test")
    assert run_predict.section_files(str(p), "training", 13, 5, 2) == train
    with pytest.raises(ValueError, match="unlabelled"):                     # any other missing section still raises
        run_predict.section_files(str(p), "unlabelled", 13, 5, 0)
    # a data list that has the section: the section, whatever the fold
    p.write_text(json.dumps({"training": items[:8], "validation": items[8:]}))
    for fold in (0, 3):
        assert run_predict.section_files(str(p), "validation", 13, 5, fold) == df.load_datalist(str(p), "validation")
