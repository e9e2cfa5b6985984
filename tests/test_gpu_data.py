"""Dataset path on the GPU: the preprocessing kernels, the slice-count voxel pick, the multi-volume gather and the
loaders against the numpy / scipy restatements of tests/dataprep_ref.py (MONAI parity unpinned), and the drivers end to
end on a small Decathlon-style task written into tmp_path."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dataprep_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(70, 81, 95), (128, 96, 64)]

# Gates of the two checks that are not bit-exact: 4 x the worst absolute error measured on an MI355X over the cases below,
# to allow for libm differences between toolchains.
#   cubed intensity vs numpy float64: measured 1.061e-07 (fp32 cbrtf + three fp32 operations on values in [0, 1])
#   trilinear resample vs scipy map_coordinates in float64, relative to the data range: measured 4.954e-08
CUBED_MEASURED, RESAMPLE_MEASURED = 1.061e-07, 4.954e-08
CUBED_GATE, RESAMPLE_GATE = 4 * CUBED_MEASURED, 4 * RESAMPLE_MEASURED


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _ct(shape, rng, chans=1, dtype=np.int16):
    v = rng.normal(-300.0, 500.0, (chans,) + shape)
    v[:, :3] = v[:, -2:] = -1024.0                      # a margin below the window: the foreground box is not the volume
    v[:, :, :4] = v[:, :, :, -5:] = -2000.0
    return np.round(v).astype(dtype) if dtype == np.int16 else v.astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("norm", [None, (0.1943, 0.2786)])
def test_intensity_prep_plain_bit_exact(shape, dtype, norm):
    from medicalsemseg_amd import hip
    rng = np.random.default_rng(7)
    src = _ct(shape, rng, 2, dtype)
    got, box = hip.intensity_prep(torch.from_numpy(src).to(_dev()), hip.INTENSITY_RANGE, -1000, 1000, norm)
    scaled = ref.scale_intensity_range(src, -1000, 1000)
    want = ref.normalize_intensity(scaled, *norm) if norm else scaled
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    b = box.cpu().tolist()
    assert (b[0], b[1], b[2], b[3] + 1, b[4] + 1, b[5] + 1) == ref.foreground_box(scaled)
    assert ref.foreground_box(scaled) != (0, 0, 0) + shape


def test_intensity_prep_copy_mode_and_empty_foreground():
    """mode NONE converts int16 to fp32 unchanged; without any voxel > 0 the box is {D, H, W, -1, -1, -1}, which the
    preprocessing reads as 'keep the whole volume'"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import preprocess_volume
    from medicalsemseg_amd.utils.arguments import get_args
    rng = np.random.default_rng(8)
    src = _ct((33, 47, 29), rng)
    got, box = hip.intensity_prep(torch.from_numpy(src).to(_dev()))
    assert np.array_equal(got.cpu().numpy(), src.astype(np.float32))
    b = box.cpu().tolist()
    assert (b[0], b[1], b[2], b[3] + 1, b[4] + 1, b[5] + 1) == ref.foreground_box(src.astype(np.float32))
    dark = np.full((1, 33, 47, 29), -1500, dtype=np.int16)
    got, box = hip.intensity_prep(torch.from_numpy(dark).to(_dev()), hip.INTENSITY_RANGE, -1000, 1000)
    assert box.cpu().tolist() == [33, 47, 29, -1, -1, -1] and float(got.abs().max()) == 0.0
    cfg = get_args(["--vol_size", "16", "--t_fixed_ct_intensity", "--t_crop_foreground_img", "--t_spatial_pad"])
    rec = preprocess_volume(dark, np.zeros((33, 47, 29), np.uint8), np.eye(4), cfg, _dev())
    assert tuple(rec["img"].shape) == (1, 33, 47, 29) and np.array_equal(rec["affine"], np.eye(4))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_intensity_prep_cubed_within_measured_gate(shape, dtype):
    from medicalsemseg_amd import hip
    rng = np.random.default_rng(9)
    src = _ct(shape, rng, 1, dtype)
    got, box = hip.intensity_prep(torch.from_numpy(src).to(_dev()), hip.INTENSITY_CUBED, -1000, 1000)
    want = ref.scale_cubed_intensity_range64(src, -1000, 1000)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"cubed intensity {shape} {np.dtype(dtype).name}: worst abs error {err:.3e} (gate {CUBED_GATE:.3e})")
    assert err <= CUBED_GATE
    sub, div = 0.1943, 0.2786
    got_n, _ = hip.intensity_prep(torch.from_numpy(src).to(_dev()), hip.INTENSITY_CUBED, -1000, 1000, (sub, div))
    # the normalisation itself is exact fp32 arithmetic on the scaled values
    assert np.array_equal(got_n.cpu().numpy(), ref.normalize_intensity(got.cpu().numpy(), sub, div))
    # the box: voxels the float64 restatement puts clearly above zero are inside, clearly-zero ones decide nothing
    b = box.cpu().tolist()
    assert (b[0], b[1], b[2], b[3] + 1, b[4] + 1, b[5] + 1) == ref.foreground_box(got.cpu().numpy())


@pytest.mark.parametrize("shape,old,new", [((70, 81, 95), (1.5, 0.8, 0.8), (1.0, 1.0, 1.0)),
                                           ((128, 96, 64), (0.7, 0.7, 2.5), (1.5, 1.5, 1.5)),
                                           ((40, 52, 44), (1.0, 1.0, 1.0), (0.5, 0.8, 2.0))])
def test_resample_spacing_vs_scipy(shape, old, new):
    from medicalsemseg_amd import data_files as df, hip
    rng = np.random.default_rng(10)
    img = rng.normal(0.0, 400.0, (2,) + shape).astype(np.float32)
    lab = rng.integers(0, 5, shape).astype(np.uint8)
    out = [df.resample_shape(n, o, w) for n, o, w in zip(shape, old, new)]
    assert out == [ref.resample_shape(n, o, w) for n, o, w in zip(shape, old, new)]
    ratio = [w / o for o, w in zip(old, new)]
    got_l = hip.resample_spacing(torch.from_numpy(lab[None]).to(_dev()), out, ratio)[0]
    assert np.array_equal(got_l.cpu().numpy(), ref.resample_label(lab, out, ratio))
    got = hip.resample_spacing(torch.from_numpy(img).to(_dev()), out, ratio).cpu().numpy()
    want = ref.resample_image64(img, out, ratio)
    err = float(np.abs(got.astype(np.float64) - want).max() / (float(img.max()) - float(img.min())))
    print(f"resample {shape} {old}->{new}: worst abs error / data range {err:.3e} (gate {RESAMPLE_GATE:.3e})")
    assert got.shape == want.shape and err <= RESAMPLE_GATE


@pytest.mark.parametrize("shape", SHAPES)
def test_resample_identity_spacing_copies_bit_for_bit(shape):
    from medicalsemseg_amd import hip
    rng = np.random.default_rng(11)
    img = rng.normal(0.0, 400.0, (1,) + shape).astype(np.float32)
    lab = rng.integers(0, 5, shape).astype(np.uint8)
    got = hip.resample_spacing(torch.from_numpy(img).to(_dev()), shape, (1.0, 1.0, 1.0))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), img.view(np.uint32))
    got_l = hip.resample_spacing(torch.from_numpy(lab[None]).to(_dev()), shape, (1.0, 1.0, 1.0))
    assert np.array_equal(got_l.cpu().numpy()[0], lab)


@pytest.mark.parametrize("shape,box,roi", [((70, 81, 95), (3, 4, 0, 68, 81, 90), 96),       # every axis padded
                                           ((128, 96, 64), (10, 0, 5, 128, 96, 60), 96),   # one axis smaller than the roi
                                           ((70, 81, 95), (0, 0, 0, 70, 81, 95), 32),      # nothing to do
                                           ((40, 52, 44), (7, 8, 9, 8, 51, 30), None)])    # crop only
def test_crop_pad_copy_bit_exact(shape, box, roi):
    from medicalsemseg_amd import hip
    rng = np.random.default_rng(12)
    img = rng.standard_normal((3,) + shape).astype(np.float32)
    lab = rng.integers(0, 9, shape).astype(np.uint8)
    ms = (roi,) * 3 if roi else None
    got, before = hip.crop_pad_copy(torch.from_numpy(img).to(_dev()), box, ms, -0.697)
    want = ref.crop_pad(img, box, ms, np.float32(-0.697))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    got_l, before_l = hip.crop_pad_copy(torch.from_numpy(lab[None]).to(_dev()), box, ms, 0)
    assert np.array_equal(got_l.cpu().numpy(), ref.crop_pad(lab[None], box, ms, 0)) and before == before_l
    n = [box[3 + a] - box[a] for a in range(3)]
    assert before == tuple((max(n[a], roi or 0) - n[a]) // 2 for a in range(3))
    with pytest.raises(hip.MssegError, match="crop_pad_copy"):
        hip.crop_pad_copy(torch.from_numpy(lab[None]).to(_dev()), (0, 0, 0, shape[0] + 1, shape[1], shape[2]), ms, 0)


def _three_volumes(rng, chans=1):
    """three cached volumes of different non-cubic sizes; the third has no foreground"""
    vols = []
    for k, shape in enumerate([(70, 81, 95), (128, 96, 64), (66, 70, 90)]):
        img = rng.standard_normal((chans,) + shape).astype(np.float32)
        lab = np.zeros(shape, dtype=np.uint8)
        if k == 0:
            lab[5:30, 40:70, 10:60] = 1
            lab[50:69, 0:9, 80:95] = 2
        elif k == 1:
            lab[100:128, 20:40, 0:7] = 3
            lab[rng.random(shape) < 0.001] = 1
        vols.append((img, lab))
    return vols


def _records(vols, dev):
    return [{"img": torch.from_numpy(i).to(dev), "lab": torch.from_numpy(l).to(dev), "affine": np.diag([1.0 + k, 1, 1, 1]),
             "original_affine": np.diag([2.0 + k, 1, 1, 1]), "filename": f"/data/vol{k}.nii.gz"} for k, (i, l) in enumerate(vols)]


def test_slab_counts_and_pick_voxels_match_nonzero_lists():
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import PICK_BG, PICK_FG, PICK_VOXEL, PickRow, VolumeDesc, _upload
    from oracle.augment import correct_crop_center
    dev = _dev()
    rng = np.random.default_rng(13)
    vols = _three_volumes(rng)
    recs = _records(vols, dev)
    thr, roi = 0.25, 48
    lists, cums = [], []
    for (img, lab), r in zip(vols, recs):
        c = hip.slab_counts(r["img"], r["lab"], thr).cpu().numpy()
        assert c.dtype == np.int32 and np.array_equal(c, ref.slab_counts(img[0], lab, thr))
        fl = lab.reshape(-1)
        lists.append((np.nonzero((fl == 0) & (img[0].reshape(-1) > thr))[0], np.nonzero(fl > 0)[0]))
        cums.append((np.cumsum(c[:, 1].astype(np.int64)), np.cumsum(c[:, 0].astype(np.int64))))
    assert lists[2][1].size == 0 and lists[2][0].size > 0
    desc = _upload([VolumeDesc(r["img"].data_ptr(), r["lab"].data_ptr(), *r["img"].shape) for r in recs], dev)
    rows, want = [], []
    for i in range(200):
        vi = i % 3
        use_fg = int(i % 2 == 0 and lists[vi][1].size > 0)
        lst, cum = lists[vi][use_fg], cums[vi][use_fg]
        idx = int(rng.integers(0, lst.size)) if i >= 12 else (0, lst.size - 1)[i % 4 < 2]      # first and last candidates too
        z = int(np.searchsorted(cum, idx, side="right"))
        rows.append(PickRow(vi, PICK_FG if use_fg else PICK_BG, z, idx - (int(cum[z - 1]) if z else 0), 0, 0, 0.0, 1.0))
        want.append(int(lst[idx]))
    rows.append(PickRow(1, PICK_VOXEL, 127, 95 * 64 + 63, 0, 0, 0.0, 1.0))          # explicit voxel: the far corner
    want.append(128 * 96 * 64 - 1)
    out = torch.empty(len(rows), 8, dtype=torch.int32, device=dev)
    hip.pick_voxels(desc, 3, _upload(rows, dev), len(rows), roi, thr, out)
    out = out.cpu().numpy()
    for row, flat, o in zip(rows, want, out):
        D, H, W = vols[row.vol][1].shape
        assert int(o[6]) * H * W + int(o[7]) == flat
        c = correct_crop_center((flat // (H * W), (flat // W) % H, flat % W), (roi,) * 3, (D, H, W))
        assert tuple(o[:3]) == c and tuple(o[3:6]) == tuple(v - roi // 2 for v in c)
        assert all(0 <= s and s + roi <= n for s, n in zip(o[3:6], (D, H, W)))
    # a rank beyond the slice's count is reported, the centre still keeps the roi inside
    bad = torch.empty(1, 8, dtype=torch.int32, device=dev)
    hip.pick_voxels(desc, 3, _upload([PickRow(2, PICK_FG, 3, 0, 0, 0, 0.0, 1.0)], dev), 1, roi, thr, bad)
    bad = bad.cpu().tolist()[0]
    assert bad[7] == -1 and all(0 <= s and s + roi <= n for s, n in zip(bad[3:6], vols[2][1].shape))


@pytest.mark.parametrize("chans", [1, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("roi", [32, 30])
def test_aug_crop_multi_bit_exact_vs_oracle_in_one_launch(chans, dtype, roi, monkeypatch):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow, VolumeDesc, _upload
    from oracle.augment import apply_row
    dev = _dev()
    rng = np.random.default_rng(14)
    vols = _three_volumes(rng, chans)
    recs = _records(vols, dev)
    desc = _upload([VolumeDesc(r["img"].data_ptr(), r["lab"].data_ptr(), *r["img"].shape) for r in recs], dev)
    rows, picks = [], []
    for i in range(12):
        vi = i % 3
        start = [int(rng.integers(0, n - roi + 1)) for n in vols[vi][1].shape]
        if i == 5:
            start = [n - roi for n in vols[vi][1].shape]
        flips, rotk = (i * 3 + 1) % 8 if i < 8 else i % 8, (i + i // 4) % 4          # all 8 masks, all 4 turns
        rows.append(PickRow(vi, PICK_VOXEL, 0, 0, flips, rotk, float(rng.uniform(-0.1, 0.1)), 1.0 + float(rng.uniform(-0.1, 0.1))))
        picks.append([s + roi // 2 for s in start] + start + [0, 0])
    assert {r.flips for r in rows} == set(range(8)) and {r.rotk for r in rows} == {0, 1, 2, 3}
    calls = []
    real = hip.lib().msseg_aug_crop_multi
    monkeypatch.setattr(hip, "lib", lambda: type("L", (), {"msseg_aug_crop_multi": staticmethod(lambda *a: calls.append(1) or real(*a)),
                                                          "msseg_last_error": hip.load_library().msseg_last_error})())
    img = torch.empty(12, chans, roi, roi, roi, dtype=dtype, device=dev)
    lab = torch.empty(12, 1, roi, roi, roi, dtype=torch.float32, device=dev)
    hip.aug_crop_multi(desc, 3, _upload(rows, dev), torch.tensor(picks, dtype=torch.int32, device=dev), img, lab, roi)
    monkeypatch.undo()
    assert len(calls) == 1                                                           # one launch for 12 rows over 3 volumes
    for j, (row, p) in enumerate(zip(rows, picks)):
        vi, fl = row.vol, (row.flips & 1, row.flips & 2, row.flips & 4)
        wi, wl = apply_row(vols[vi][0], vols[vi][1], tuple(p[3:6]), roi, fl, row.rotk, row.shift, row.scale)
        want = torch.from_numpy(wi).to(dtype)                                        # bf16: the fp32 result rounded once
        assert torch.equal(img[j].cpu(), want), j
        assert np.array_equal(lab[j, 0].cpu().numpy(), wl), j


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_aug_crop_multi_equals_aug_crop_batch_on_one_volume(dtype):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import PICK_VOXEL, AugRow, PickRow, VolumeDesc, _upload
    dev = _dev()
    rng = np.random.default_rng(15)
    img = torch.from_numpy(rng.standard_normal((2, 70, 81, 95)).astype(np.float32)).to(dev)
    lab = torch.from_numpy(rng.integers(0, 4, (70, 81, 95)).astype(np.uint8)).to(dev)
    roi, n = 48, 8
    old_rows, new_rows, picks = [], [], []
    for i in range(n):
        s = [int(rng.integers(0, d - roi + 1)) for d in lab.shape]
        fl, rk, sh, sc = i % 8, i % 4, float(rng.uniform(-0.1, 0.1)), 1.0 + float(rng.uniform(-0.1, 0.1))
        old_rows.append(AugRow(*s, fl, rk, 0, sh, sc))
        new_rows.append(PickRow(0, PICK_VOXEL, 0, 0, fl, rk, sh, sc))
        picks.append([v + roi // 2 for v in s] + s + [0, 0])
    a_i = torch.empty(n, 2, roi, roi, roi, dtype=dtype, device=dev)
    a_l = torch.empty(n, 1, roi, roi, roi, dtype=torch.float32, device=dev)
    b_i, b_l = torch.empty_like(a_i), torch.empty_like(a_l)
    hip.aug_crop_batch(img, lab, _upload(old_rows, dev), a_i, a_l, roi)
    desc = _upload([VolumeDesc(img.data_ptr(), lab.data_ptr(), *img.shape)], dev)
    hip.aug_crop_multi(desc, 1, _upload(new_rows, dev), torch.tensor(picks, dtype=torch.int32, device=dev), b_i, b_l, roi)
    assert torch.equal(a_i, b_i) and torch.equal(a_l, b_l)


def _batches(loader):
    out = []
    for b in loader:
        out.append((b["image"].clone(), b["label"].clone(), list(b["image_meta_dict"]["filename_or_obj"]),
                    torch.stack(b["image_transforms"][0]["extra_info"]["center"], 1).clone(),
                    torch.stack(b["image_transforms"][0]["orig_size"], 1).clone(), b["image_meta_dict"]["affine"].clone(),
                    b["image_meta_dict"]["original_affine"].clone(), b["image_transforms"][0]))
    return out


@pytest.mark.parametrize("crop", ["fgbg", "spatial"])
def test_device_dataset_loader_is_seeded_and_visits_every_volume(crop):
    from medicalsemseg_amd.data_device import DeviceDatasetLoader
    from medicalsemseg_amd.utils import misc
    from oracle.augment import apply_row
    dev = _dev()
    vols = _three_volumes(np.random.default_rng(16))
    recs = _records(vols, dev)
    roi, ppi, batch = 32, 2, 3
    n_batches = len(recs) * ppi // batch                                             # one epoch
    kw = dict(patches_per_image=ppi, device=dev, seed=21, crop=crop, pos=2.0, neg=1.0, flip_prob=0.5, rot_prob=0.6,
              shift_prob=0.5, scale_prob=0.5, image_threshold=0.0)
    a = DeviceDatasetLoader(recs, roi, batch, n_batches, **kw)
    b = DeviceDatasetLoader(recs, roi, batch, n_batches, **kw)
    for epoch in range(2):
        ba, bb = _batches(a), _batches(b)
        assert len(ba) == n_batches == len(a)
        names = []
        for x, y in zip(ba, bb):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2] == y[2] and torch.equal(x[3], y[3])
            names += x[2]
        # every volume once per epoch, patches_per_image consecutive samples from the same file
        assert sorted(names[::ppi]) == sorted(r["filename"] for r in recs)
        assert all(names[i] == names[i - i % ppi] for i in range(len(names)))
    assert a.launches == 2 * n_batches                                               # one gather launch per batch
    c = DeviceDatasetLoader(recs, roi, batch, n_batches, **dict(kw, seed=22))
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(_batches(c), ba))
    # the last batch against the oracle, with the meta of each sample's own volume
    by_name = {r["filename"]: k for k, r in enumerate(recs)}
    img, lab, names, cen, osz, aff, oaff, tr = ba[-1]
    for j, row in enumerate(a.last_rows):
        k = by_name[names[j]]
        assert row.vol == k and tuple(osz[j].tolist()) == vols[k][1].shape
        assert float(aff[j, 0, 0]) == 1.0 + k and float(oaff[j, 0, 0]) == 2.0 + k
        start = tuple(int(v) for v in a.last_picks[j, 3:6])
        assert tuple(int(v) - roi // 2 for v in cen[j]) == start
        wi, wl = apply_row(vols[k][0], vols[k][1], start, roi, (row.flips & 1, row.flips & 2, row.flips & 4), row.rotk,
                           row.shift, row.scale)
        assert np.array_equal(img[j].cpu().numpy(), wi) and np.array_equal(lab[j, 0].cpu().numpy(), wl)
        if crop == "fgbg" and row.mode == 1:
            flat = int(a.last_picks[j, 6]) * vols[k][1].shape[1] * vols[k][1].shape[2] + int(a.last_picks[j, 7])
            assert vols[k][1].reshape(-1)[flat] > 0                                  # a foreground pick is a foreground voxel
    rel = misc.get_rel_crop_loc(tr)
    assert tuple(rel.shape) == (batch, 3) and float(rel.min()) > 0 and float(rel.max()) < 1


def test_unimplemented_flags_name_themselves():
    from medicalsemseg_amd.data_device import DeviceDatasetLoader, check_transform_flags, crop_mode
    from medicalsemseg_amd.utils.arguments import get_args
    for flag in ("t_rand_crop_classes", "t_rand_crop_dilated_center", "t_convert_labels_to_brats", "t_percentile_ct_intensity"):
        with pytest.raises(NotImplementedError, match=flag):
            check_transform_flags(get_args(["--" + flag]))
    with pytest.raises(NotImplementedError, match="t_normalize_channel_wise"):
        check_transform_flags(get_args(["--t_normalize", "--t_normalize_channel_wise"]))
    with pytest.raises(SystemExit, match="t_rand_crop_fgbg.*t_rand_spatial_crop.*t_rand_crop_classes"):
        crop_mode(get_args([]))
    with pytest.raises(NotImplementedError):
        DeviceDatasetLoader(_records(_three_volumes(np.random.default_rng(1)), _dev()), 32, 2, 1, device=_dev(), crop="classes")


def test_preprocess_volume_matches_the_restated_chain():
    """orientation (LPS file) -> spacing -> fixed CT window -> foreground crop -> pad, against the restatement chained the
    same way; the affine keeps every voxel's world position"""
    from medicalsemseg_amd import data_files as df
    from medicalsemseg_amd.data_device import preprocess_volume
    from medicalsemseg_amd.utils.arguments import get_args
    dev = _dev()
    rng = np.random.default_rng(17)
    shape = (40, 72, 60)
    img = _ct(shape, rng)
    lab = ref.ellipsoid_labels(shape, 3)
    aff = np.diag([-1.5, -0.8, 0.8, 1.0])
    aff[:3, 3] = (30.0, 20.0, 10.0)
    cfg = get_args(["--vol_size", "64", "--t_voxel_spacings", "--t_voxel_dims", "1.0", "1.0", "1.0", "--t_fixed_ct_intensity",
                    "--t_crop_foreground_img", "--t_spatial_pad", "--t_normalize"])
    rec = preprocess_volume(img, lab, aff, cfg, dev, "x.nii.gz")
    # the restated chain
    i0, l0 = np.flip(img.astype(np.float32), (1, 2)), np.flip(lab, (0, 1))
    ratio = [1.0 / 1.5, 1.25, 1.25]
    out = [ref.resample_shape(n, o, 1.0) for n, o in zip(shape, (1.5, 0.8, 0.8))]
    l1 = ref.resample_label(l0, out, ratio)
    i1 = ref.resample_image64(i0, out, ratio)
    scaled = ref.scale_intensity_range(i1.astype(np.float32), -1000, 1000)
    got = rec["img"].cpu().numpy()
    D, H, W = got.shape[1:]
    assert min(D, H, W) >= 64 and rec["lab"].shape == (D, H, W)
    # the box: fp32 vs float64 interpolation may disagree on voxels the clip holds within rounding of 0, so the product's
    # box is checked to be the restatement's up to such voxels, then used for the comparison of the contents
    box, before = rec["box"], rec["pad_before"]
    fb_lo = ref.foreground_box(np.where(scaled > 1e-5, scaled, 0))
    fb_hi = ref.foreground_box(np.where(scaled > 0, 1.0, 0) + (i1 > -1000.01))
    assert all(fb_hi[k] <= box[k] <= fb_lo[k] and fb_lo[3 + k] <= box[3 + k] <= fb_hi[3 + k] for k in range(3))
    assert box != (0, 0, 0) + tuple(out) and before == tuple((64 - (box[3 + k] - box[k])) // 2 for k in range(3))
    # the affine: unit spacing, RAS, and voxel 0 of the cached volume sits where the crop (minus the padding) starts
    a = rec["affine"]
    assert np.allclose(df.spacing_of(a), 1.0) and all(a[o, o] > 0 for o in range(3))
    res_aff = df.rescale_affine(df.reorient_affine(aff, shape, (0, 1, 2), (True, True, False)), ratio)
    assert np.allclose(a[:, 3], res_aff @ np.array([box[0] - before[0], box[1] - before[1], box[2] - before[2], 1.0]))
    assert np.array_equal(rec["original_affine"], aff)
    pad = float((np.float32(0) - np.float32(cfg.t_norm_mean)) / np.float32(cfg.t_norm_std))
    want = ref.crop_pad(ref.normalize_intensity(scaled, cfg.t_norm_mean, cfg.t_norm_std), box, (64,) * 3, np.float32(pad))
    assert want.shape == got.shape
    # resampled values of magnitude <= 4e3 carry a few fp32 ulps (2.4e-4 each); / 2000 for the window, / 0.2786 for the
    # normalisation: a few times 4.4e-7, plus the fp32 roundings of values of order 1 to 4 -> 5e-6
    assert float(np.abs(want - got).max()) <= 5e-6
    assert np.array_equal(rec["lab"].cpu().numpy(), ref.crop_pad(l1[None], box, (64,) * 3, 0)[0])


# ---- drivers end to end ---------------------------------------------------------------------------------------------
TRAIN_FLAGS = ["--model", "UNetSmall", "--output_dim", "2", "--vol_size", "32", "--t_voxel_spacings", "--t_voxel_dims", "1.0",
               "1.0", "1.0", "--t_fixed_ct_intensity", "--t_crop_foreground_img", "--t_spatial_pad", "--t_rand_crop_fgbg",
               "--t_n_patches_per_image", "2", "--t_flip_prob", "0.5", "--t_rot_prob", "0.5", "--n_images_per_batch", "2",
               "--json_list", "dataset.json", "--task", "Task99_CT"]


@pytest.fixture
def ct_task(tmp_path):
    items = ref.write_ct_dataset(str(tmp_path / "data" / "Task99_CT"), n=6, n_cls=2)
    return str(tmp_path / "data"), items


def _split(data_path, fold=0):
    from medicalsemseg_amd import data_files as df
    files = df.load_datalist(os.path.join(data_path, "Task99_CT", "dataset.json"), "training")
    return df.cv_split(files, 13, 5, fold)


def _train_cmd(data_path, out):
    return [os.path.join(ROOT, "run_training.py"), *TRAIN_FLAGS, "--data_path", data_path, "--epochs", "2", "--val_interval", "2",
            "--warmup_epochs", "1", "--output_dir", out, "--save_ckpt_freq", "2"]


def test_run_training_and_evaluation_on_files(ct_task, tmp_path):
    data_path, _ = ct_task
    train, val = _split(data_path)
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, *_train_cmd(data_path, out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"Number of files in training cv split: {len(train)}" in r.stdout
    assert f"Number of files in val cv split: {len(val)}" in r.stdout
    m = re.search(r"rank 0: training partition (\d+) file\(s\) \[([^\]]*)\], validation partition (\d+) file", r.stdout)
    assert m and int(m.group(1)) == len(train) and int(m.group(3)) == len(val)
    assert m.group(2).split(", ") == [os.path.basename(f["image"]) for f in train]
    log = [json.loads(l) for l in open(os.path.join(out, "log.txt"))]
    assert len(log) == 2 and all(np.isfinite(e["train/loss"]) for e in log), log
    ck = os.path.join(out, "checkpoint-1.pth")
    assert os.path.exists(ck) or os.path.exists(os.path.join(out, "best_model.pth"))
    ev_out = str(tmp_path / "ev")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_evaluation.py"), *TRAIN_FLAGS, "--data_path", data_path, "--resume",
                        ck, "--output_dir", ev_out], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ev = json.load(open(os.path.join(ev_out, "eval.json")))
    key = "val/mDice" if "val/mDice" in ev else "eval/mDice"
    assert 0.0 <= ev[key] <= 1.0 and f"validation partition {len(val)} of {len(val)} file(s)" in r.stdout


def test_run_training_on_files_two_ranks_share_one_gpu_over_gloo(ct_task, tmp_path):
    data_path, _ = ct_task
    train, _ = _split(data_path)
    env = dict(os.environ, MSSEG_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29900 + os.getpid() % 300
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), *_train_cmd(data_path, str(tmp_path / "out")), "--backend", "gloo"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    parts = {int(m.group(1)): m.group(2).split(", ")
             for m in re.finditer(r"rank (\d): training partition \d+ file\(s\) \[([^\]]*)\]", r.stdout)}
    assert set(parts) == {0, 1} and len(parts[0]) == len(parts[1]) == (len(train) + 1) // 2
    names = [os.path.basename(f["image"]) for f in train]
    if len(train) % 2 == 0:
        assert not set(parts[0]) & set(parts[1])
    assert parts[0] == (names + names[:len(names) % 2])[0::2] and parts[1] == (names + names[:len(names) % 2])[1::2]
    assert set(parts[0]) | set(parts[1]) == set(names)


def test_run_training_without_a_crop_flag_names_the_three_flags(ct_task, tmp_path):
    data_path, _ = ct_task
    flags = [f for f in TRAIN_FLAGS if f != "--t_rand_crop_fgbg"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_training.py"), *flags, "--data_path", data_path, "--epochs", "1",
                        "--output_dir", str(tmp_path / "out")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert all(f in r.stderr for f in ("--t_rand_crop_fgbg", "--t_rand_spatial_crop", "--t_rand_crop_classes"))


# ---- background candidates under --t_normalize, invalid gather rows ---------------------------------------------------
def test_background_candidates_under_normalisation_are_those_of_scaled_above_zero():
    """The reference thresholds the background crop centres at 0 on the scaled, un-normalised image
    (RandCropByPosNegLabeld in front of NormalizeIntensityd).  The cache holds the normalised image, so the threshold is the
    normalised zero: per-slice counts and picked voxels must be those of `scaled > 0`, padding excluded."""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import PICK_BG, DeviceDatasetLoader, normalised_zero, preprocess_volume
    from medicalsemseg_amd.utils.arguments import get_args
    dev = _dev()
    rng = np.random.default_rng(18)
    shape = (40, 72, 60)
    img = _ct(shape, rng)                                  # int16 HU around -300 +- 500: many voxels in (-1000, -611] HU
    lab = ref.ellipsoid_labels(shape, 3)
    flags = ["--vol_size", "64", "--t_fixed_ct_intensity", "--t_crop_foreground_img", "--t_spatial_pad"]
    cfg_n, cfg_0 = get_args(flags + ["--t_normalize"]), get_args(flags)
    rec_n = preprocess_volume(img, lab, np.eye(4), cfg_n, dev, "n.nii.gz")
    rec_0 = preprocess_volume(img, lab, np.eye(4), cfg_0, dev, "0.nii.gz")
    assert rec_n["box"] == rec_0["box"] and rec_n["pad_before"] == rec_0["pad_before"] and max(rec_n["pad_before"]) > 0
    scaled, lab_c = rec_0["img"].cpu().numpy(), rec_0["lab"].cpu().numpy()
    assert np.array_equal(rec_n["img"].cpu().numpy(), ref.normalize_intensity(scaled, cfg_n.t_norm_mean, cfg_n.t_norm_std))
    thr = normalised_zero(cfg_n)
    assert thr < 0 and normalised_zero(cfg_0) == 0.0
    want = ref.slab_counts(scaled[0], lab_c, 0.0)
    low = (lab_c == 0) & (scaled[0] > 0) & (scaled[0] <= cfg_n.t_norm_mean)
    assert low.sum() > 1000                               # the voxels a threshold of 0 on the normalised image would lose
    got = hip.slab_counts(rec_n["img"], rec_n["lab"], thr).cpu().numpy()
    assert np.array_equal(got, want)
    assert got[:, 1].sum() > hip.slab_counts(rec_n["img"], rec_n["lab"], 0.0).cpu().numpy()[:, 1].sum()
    # the loader with that threshold draws its background centres from exactly that set
    ld = DeviceDatasetLoader([rec_n], 32, 8, 6, device=dev, seed=3, pos=1.0, neg=3.0, image_threshold=thr)
    assert int(ld.cum[0][1][-1]) == int(want[:, 1].sum()) and int(ld.cum[0][0][-1]) == int(want[:, 0].sum())
    H, W = lab_c.shape[1:]
    seen_low = n_bg = 0
    for _ in ld:
        for row, p in zip(ld.last_rows, ld.last_picks.tolist()):
            if row.mode == PICK_BG:
                z, yx = p[6], p[7]
                assert yx >= 0 and lab_c[z, yx // W, yx % W] == 0 and scaled[0, z, yx // W, yx % W] > 0
                seen_low += bool(low[z, yx // W, yx % W])
                n_bg += 1
    assert n_bg >= 20 and seen_low > 0


def test_aug_crop_multi_invalid_rows_give_zero_patches():
    """rows that name no volume, a volume with another channel count or one smaller than the roi: nothing is read, the
    patch is all zero, the other rows of the batch are untouched"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow, VolumeDesc, _upload
    from oracle.augment import apply_row
    dev = _dev()
    rng = np.random.default_rng(19)
    roi = 32
    big = (rng.standard_normal((1, 40, 44, 48)).astype(np.float32), rng.integers(0, 3, (40, 44, 48)).astype(np.uint8))
    small = (rng.standard_normal((1, 40, 20, 48)).astype(np.float32), np.zeros((40, 20, 48), np.uint8))
    two = (rng.standard_normal((2, 40, 44, 48)).astype(np.float32), np.zeros((40, 44, 48), np.uint8))
    t = [(torch.from_numpy(i).to(dev), torch.from_numpy(l).to(dev)) for i, l in (big, small, two)]
    desc = _upload([VolumeDesc(i.data_ptr(), l.data_ptr(), *i.shape) for i, l in t], dev)
    vols = [0, 1, 2, 3, -1, 0]
    rows = [PickRow(v, PICK_VOXEL, 0, 0, 5, 1, 0.05, 1.1) for v in vols]
    picks = torch.tensor([[20, 20, 20, 4, 4, 4, 0, 0]] * len(rows), dtype=torch.int32, device=dev)
    for dtype in (torch.float32, torch.bfloat16):
        img = torch.full((len(rows), 1, roi, roi, roi), 7.0, dtype=dtype, device=dev)
        lab = torch.full((len(rows), 1, roi, roi, roi), 7.0, dtype=torch.float32, device=dev)
        hip.aug_crop_multi(desc, 3, _upload(rows, dev), picks, img, lab, roi)
        wi, wl = apply_row(big[0], big[1], (4, 4, 4), roi, (1, 0, 4), 1, 0.05, 1.1)
        for j, v in enumerate(vols):
            if v == 0:
                assert torch.equal(img[j].cpu(), torch.from_numpy(wi).to(dtype)) and np.array_equal(lab[j, 0].cpu().numpy(), wl)
            else:
                assert float(img[j].float().abs().max()) == 0.0 and float(lab[j].abs().max()) == 0.0, (j, v)
