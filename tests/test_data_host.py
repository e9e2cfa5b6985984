"""Host side of the dataset path (no GPU): data list, cross-validation split, per-rank partition, the NIfTI reader on real
header variants, orientation to RAS and the resampled shape rule."""
import json
import os
import random

import numpy as np
import pytest

from medicalsemseg_amd import data_files as df
from medicalsemseg_amd.utils.nifti import load_nifti, save_nifti
from tests.dataprep_ref import write_nifti_raw


def _files(n):
    return [{"image": f"/d/img{i}.nii.gz", "label": f"/d/lab{i}.nii.gz"} for i in range(n)]


@pytest.mark.parametrize("world", [2, 3])
def test_partition_even_divisible_pads_from_the_head(world):
    files = _files(7)
    parts = [df.partition(files, world, r) for r in range(world)]
    assert len({len(p) for p in parts}) == 1 and len(parts[0]) == -(-7 // world)
    assert {f["image"] for p in parts for f in p} == {f["image"] for f in files}
    padded = files + files[:world * len(parts[0]) - 7]
    for r in range(world):
        assert parts[r] == padded[r::world]
    # without the padding the partitions are the plain strides
    assert [len(df.partition(files, world, r, even_divisible=False)) for r in range(world)] == [len(files[r::world]) for r in range(world)]


def test_partition_single_rank_and_more_ranks_than_files():
    files = _files(3)
    assert df.partition(files, 1, 0) == files
    parts = [df.partition(files[:2], 5, r) for r in range(5)]
    assert all(len(p) == 1 for p in parts)
    assert [p[0] for p in parts] == [files[0], files[1], files[0], files[1], files[0]]


@pytest.mark.parametrize("fold", range(5))
def test_cv_split_matches_the_literal_recomputation(fold):
    files = _files(23)
    train, val = df.cv_split(files, 13, 5, fold)
    lit = list(files)
    random.Random(13).shuffle(lit)
    splits = np.array_split(lit, 5)
    folds = list(range(5))
    folds.pop(fold)
    want_train = [f for i in folds for f in splits[i]]
    assert train == want_train and val == list(splits[fold])
    assert len(train) + len(val) == 23 and not {f["image"] for f in train} & {f["image"] for f in val}
    assert files == _files(23)                                   # the caller's list is not shuffled in place


def test_load_datalist_resolves_relative_and_absolute_paths(tmp_path):
    task = tmp_path / "Task99_X"
    task.mkdir()
    abs_img = str(tmp_path / "elsewhere" / "b.nii.gz")
    js = {"training": [{"image": "./imagesTr/a.nii.gz", "label": "./labelsTr/a.nii.gz"},
                       {"image": abs_img, "label": "labelsTr/b.nii.gz"}], "test": ["./imagesTs/t.nii.gz"]}
    (task / "dataset.json").write_text(json.dumps(js))
    p = df.datalist_path(str(tmp_path), "Task99_X", "dataset.json")
    got = df.load_datalist(p, "training")
    assert got[0] == {"image": str(task / "imagesTr" / "a.nii.gz"), "label": str(task / "labelsTr" / "a.nii.gz")}
    assert got[1] == {"image": abs_img, "label": str(task / "labelsTr" / "b.nii.gz")}
    assert df.load_datalist(p, "test") == [{"image": str(task / "imagesTs" / "t.nii.gz")}]
    assert not df.has_key(p, "validation") and df.has_key(p, "training")
    with pytest.raises(ValueError, match="validation"):
        df.load_datalist(p, "validation")


def test_nifti_scaled_int16(tmp_path):
    rng = np.random.default_rng(0)
    raw = rng.integers(0, 2000, (7, 9, 5)).astype(np.int16)
    srows = np.array([[0.7, 0, 0, -3.0], [0, 0.7, 0, 4.0], [0, 0, 2.5, 5.0]])
    write_nifti_raw(tmp_path / "s.nii.gz", raw, pixdim=(0.7, 0.7, 2.5), slope=2.0, inter=-1024.0, sform_code=1, srows=srows)
    data, aff = load_nifti(str(tmp_path / "s.nii.gz"))
    assert data.dtype == np.float32 and np.array_equal(data, raw.astype(np.float32) * 2.0 - 1024.0)
    assert np.allclose(aff[:3], srows, atol=1e-6) and np.array_equal(aff[3], [0, 0, 0, 1])
    # slope 0 and the identity pair mean "no scaling": the stored dtype comes back
    for k, (sl, it) in enumerate(((0.0, 0.0), (1.0, 0.0))):
        write_nifti_raw(tmp_path / f"n{k}.nii", raw, slope=sl, inter=it, sform_code=1, srows=srows)
        d2, _ = load_nifti(str(tmp_path / f"n{k}.nii"))
        assert d2.dtype == np.int16 and np.array_equal(d2, raw)


def test_nifti_qform_only_and_pixdim_only(tmp_path):
    vol = np.arange(4 * 5 * 6, dtype=np.float32).reshape(4, 5, 6)
    # quaternion (0, 0, 1): half a turn about z -> diag(-1, -1, 1), the LPS frame of most CT files
    write_nifti_raw(tmp_path / "q.nii", vol, pixdim=(0.8, 0.9, 2.0), qform_code=1, quatern=(0.0, 0.0, 1.0),
                    qoffset=(100.0, 120.0, -50.0))
    data, aff = load_nifti(str(tmp_path / "q.nii"))
    assert np.array_equal(data, vol)
    want = np.array([[-0.8, 0, 0, 100.0], [0, -0.9, 0, 120.0], [0, 0, 2.0, -50.0], [0, 0, 0, 1.0]])
    assert np.allclose(aff, want, atol=1e-6)
    # qfac = -1 mirrors the third axis
    write_nifti_raw(tmp_path / "qf.nii", vol, pixdim=(0.8, 0.9, 2.0), qfac=-1.0, qform_code=1)
    _, aff = load_nifti(str(tmp_path / "qf.nii"))
    assert np.allclose(aff[:3, :3], np.diag([0.8, 0.9, -2.0]), atol=1e-6)
    # a quarter turn about x: quaternion (sin 45, 0, 0)
    s = np.sin(np.pi / 4)
    write_nifti_raw(tmp_path / "qx.nii", vol, pixdim=(1.0, 2.0, 3.0), qform_code=1, quatern=(s, 0.0, 0.0))
    _, aff = load_nifti(str(tmp_path / "qx.nii"))
    assert np.allclose(aff[:3, :3], np.array([[1.0, 0, 0], [0, 0, -3.0], [0, 2.0, 0]]), atol=1e-5)
    # neither form: the voxel sizes alone
    write_nifti_raw(tmp_path / "p.nii", vol, pixdim=(1.5, 0.8, 0.8))
    data, aff = load_nifti(str(tmp_path / "p.nii"))
    assert np.array_equal(data, vol) and np.allclose(aff, np.diag([1.5, 0.8, 0.8, 1.0]), atol=1e-6)


def test_nifti_4d_channels_last_and_load_case(tmp_path):
    rng = np.random.default_rng(1)
    vol = rng.standard_normal((5, 6, 7, 4)).astype(np.float32)
    lab = rng.integers(0, 3, (5, 6, 7)).astype(np.uint8)
    aff = np.diag([1.0, 1.0, 1.0, 1.0])
    save_nifti(str(tmp_path / "m.nii.gz"), vol, aff)
    save_nifti(str(tmp_path / "l.nii.gz"), lab, aff)
    img, lb, a = df.load_case({"image": str(tmp_path / "m.nii.gz"), "label": str(tmp_path / "l.nii.gz")})
    assert img.shape == (4, 5, 6, 7) and np.array_equal(img, np.moveaxis(vol, -1, 0)) and np.array_equal(lb, lab)
    assert img.flags.c_contiguous and np.array_equal(a, aff)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
def test_save_nifti_round_trip_unchanged(tmp_path, dtype):
    rng = np.random.default_rng(2)
    vol = np.abs(rng.standard_normal((6, 7, 8)) * 50).astype(dtype)
    aff = np.array([[0.0, -1.5, 0.0, 10.0], [0.8, 0.0, 0.0, -4.0], [0.0, 0.0, 2.0, 3.0], [0, 0, 0, 1.0]])
    for ext in (".nii", ".nii.gz"):
        save_nifti(str(tmp_path / ("v" + ext)), vol, aff)
        data, a = load_nifti(str(tmp_path / ("v" + ext)))
        assert data.dtype == np.dtype(dtype) and np.array_equal(data, vol)
        assert np.array_equal(a, aff.astype(np.float32).astype(np.float64))


def _apply(vol, perm, flips):
    out = np.transpose(vol, perm)
    for ax, f in enumerate(flips):
        if f:
            out = np.flip(out, ax)
    return out


def test_orientation_lps_and_permuted_affine():
    shape = (4, 5, 6)
    lps = np.array([[-0.8, 0, 0, 50.0], [0, -0.9, 0, 60.0], [0, 0, 2.0, -7.0], [0, 0, 0, 1.0]])
    perm, flips = df.ras_orientation(lps)
    assert perm == (0, 1, 2) and flips == (True, True, False)
    # "SAR": voxel axis 0 runs to Superior, 1 to Anterior, 2 to Right (slightly oblique)
    sar = np.array([[0.02, 0.0, 0.7, 1.0], [0.0, 0.9, 0.01, 2.0], [2.5, 0.03, 0.0, 3.0], [0, 0, 0, 1.0]])
    perm2, flips2 = df.ras_orientation(sar)
    assert perm2 == (2, 1, 0) and flips2 == (False, False, False)
    ila = np.array([[0.0, -0.7, 0.0, 1.0], [0.0, 0.0, 0.9, 2.0], [-2.5, 0.0, 0.0, 3.0], [0, 0, 0, 1.0]])     # I, L, A
    perm3, flips3 = df.ras_orientation(ila)
    assert perm3 == (1, 2, 0) and flips3 == (True, False, True)
    vol = np.arange(np.prod(shape)).reshape(shape)
    for aff, p, f in ((lps, perm, flips), (sar, perm2, flips2), (ila, perm3, flips3)):
        new = df.reorient_affine(aff, shape, p, f)
        M = new[:3, :3]
        assert all(M[o, o] > 0 and abs(M[o, o]) == np.abs(M[:, o]).max() == np.abs(M[o, :]).max() for o in range(3))
        # every voxel keeps its world position
        out = _apply(vol, p, f)
        for idx in ((0, 0, 0), (1, 2, 3), tuple(s - 1 for s in out.shape)):
            src = np.argwhere(vol == out[idx])[0]
            assert np.allclose(new @ np.array([*idx, 1.0]), aff @ np.array([*src, 1.0]))
    assert np.allclose(df.spacing_of(sar), [np.sqrt(0.02 ** 2 + 2.5 ** 2), np.sqrt(0.9 ** 2 + 0.03 ** 2), np.sqrt(0.7 ** 2 + 0.01 ** 2)])


def test_resample_shape_rule_and_affine_updates():
    # round((n - 1) * old / new + 1)
    assert df.resample_shape(48, 1.5, 1.0) == 72          # 47 * 1.5 + 1 = 71.5 -> half to even
    assert df.resample_shape(64, 0.8, 1.0) == 51          # 63 * 0.8 + 1 = 51.4
    assert df.resample_shape(100, 1.0, 1.0) == 100
    assert df.resample_shape(512, 0.7, 1.5) == 239        # 511 * 0.7 / 1.5 + 1 = 239.47
    assert df.resample_shape(33, 5.0, 1.25) == 129        # up-sampling by 4: 32 * 4 + 1
    assert df.resample_shape(1, 3.0, 1.0) == 1
    aff = np.diag([1.5, 0.8, 0.8, 1.0])
    aff[:3, 3] = (1.0, 2.0, 3.0)
    new = df.rescale_affine(aff, [1.0 / 1.5, 1.25, 1.25])
    assert np.allclose(df.spacing_of(new), [1.0, 1.0, 1.0]) and np.array_equal(new[:3, 3], aff[:3, 3])
    moved = df.shift_affine(new, [2, -3, 4])
    assert np.allclose(moved[:3, 3], [3.0, -1.0, 7.0]) and np.array_equal(moved[:3, :3], new[:3, :3])


def test_voxel_dims_broadcast_and_normalised_zero():
    from medicalsemseg_amd.data_device import normalised_zero, voxel_dims
    from medicalsemseg_amd.utils.arguments import get_args
    assert voxel_dims(get_args(["--t_voxel_spacings"])) == (1.0, 1.0, 1.0)                  # the parser default, one value
    assert voxel_dims(get_args(["--t_voxel_dims", "1.5"])) == (1.5, 1.5, 1.5)
    assert voxel_dims(get_args(["--t_voxel_dims", "1.5", "0.8", "0.7"])) == (1.5, 0.8, 0.7)
    for bad in (["1.0", "2.0"], ["1.0", "0.0", "1.0"]):
        with pytest.raises(ValueError, match="--t_voxel_dims"):
            voxel_dims(get_args(["--t_voxel_dims", *bad]))
    assert normalised_zero(get_args([])) == 0.0
    want = float((np.float32(0.0) - np.float32(0.1943)) / np.float32(0.2786))
    assert normalised_zero(get_args(["--t_normalize"])) == want and -0.6975 < want < -0.6973
