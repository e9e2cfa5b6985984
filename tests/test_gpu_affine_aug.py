"""The affine crop gather on the GPU (msseg_aug_crop_affine, --t_affine_prob): identity matrices against the plain gather,
random rotations and zooms bit for bit against the numpy restatement of tests/affine_ref.py, hand-written matrices whose
result needs no restatement, the loaders and the training driver."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import affine_ref as aref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(33, 41, 36), (37, 30, 31), (31, 35, 40)]        # the third volume has no label
PAD = -0.6974
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _volumes(chans, integer=False):
    """three cached volumes of different non-cubic sizes -> (numpy (img, lab or None) list, device tensors, descriptor table)"""
    key = (chans, integer)
    if key not in _CACHE:
        from medicalsemseg_amd.data_device import VolumeDesc, _upload
        rng = np.random.default_rng(40 + chans)
        vols = []
        for k, shape in enumerate(SHAPES):
            img = rng.integers(-40, 41, (chans,) + shape).astype(np.float32) if integer else \
                rng.standard_normal((chans,) + shape).astype(np.float32)
            lab = rng.integers(0, 5, shape).astype(np.uint8) if k < 2 else None
            vols.append((img, lab))
        dev = _dev()
        tens = [(torch.from_numpy(i).to(dev), torch.from_numpy(l).to(dev) if l is not None else None) for i, l in vols]
        desc = _upload([VolumeDesc(i.data_ptr(), l.data_ptr() if l is not None else 0, *i.shape) for i, l in tens], dev)
        _CACHE[key] = (vols, tens, desc)
    return _CACHE[key]


def _rows(rng, roi, n):
    """n pick rows over the three volumes with all 8 flip masks and all 4 quarter turns; crop starts random, at the volume's
    corners for rows 0-5 (taps fall outside the volume there)"""
    from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow
    rows, picks = [], []
    for i in range(n):
        vi = i % 3
        shape = SHAPES[vi]
        start = [int(rng.integers(0, s - roi + 1)) for s in shape]
        if i < 3:
            start = [0, 0, 0]
        elif i < 6:
            start = [s - roi for s in shape]
        flips, rotk = (i * 3 + 1) % 8 if i < 8 else i % 8, (i + i // 4) % 4
        shift, scale = float(rng.uniform(-0.1, 0.1)), 1.0 + float(rng.uniform(-0.1, 0.1))
        rows.append(PickRow(vi, PICK_VOXEL, 0, 0, flips, rotk, shift, scale))
        picks.append([s + roi // 2 for s in start] + start + [0, 0])
    return rows, picks


def _run(desc, nvol, rows, picks, mats, chans, roi, dtype, pad=PAD, fill=None):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import _upload
    dev = _dev()
    n = len(rows)
    img = torch.full((n, chans, roi, roi, roi), 7.0 if fill is None else fill, dtype=dtype, device=dev)
    lab = torch.full((n, 1, roi, roi, roi), 7.0 if fill is None else fill, dtype=torch.float32, device=dev)
    m = torch.from_numpy(np.ascontiguousarray(np.asarray(mats, dtype=np.float64).reshape(n, 3, 3))).to(dev)
    hip.aug_crop_affine(desc, nvol, _upload(rows, dev), torch.tensor(picks, dtype=torch.int32, device=dev), m, img, lab, roi, pad)
    return img, lab


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("chans", [1, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("roi", [16, 30])
def test_identity_matrices_are_bit_identical_to_aug_crop_multi(chans, dtype, roi):
    """roi 16 takes the old kernel's vector path, roi 30 its scalar tail; all flip masks, all quarter turns"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import _upload
    dev = _dev()
    vols, tens, desc = _volumes(chans)
    rows, picks = _rows(np.random.default_rng(41), roi, 16)
    assert {r.flips for r in rows} == set(range(8)) and {r.rotk for r in rows} == {0, 1, 2, 3}
    # the old kernel leaves the label of a volume without a label map untouched: both start from zeros
    got_i, got_l = _run(desc, 3, rows, picks, np.tile(np.eye(3), (16, 1, 1)), chans, roi, dtype, fill=0.0)
    old_i = torch.zeros_like(got_i)
    old_l = torch.zeros_like(got_l)
    hip.aug_crop_multi(desc, 3, _upload(rows, dev), torch.tensor(picks, dtype=torch.int32, device=dev), old_i, old_l, roi)
    assert torch.equal(_bits(got_i), _bits(old_i)) and torch.equal(_bits(got_l), _bits(old_l))
    assert float(got_i.float().abs().max()) > 0 and float(got_l.max()) > 0


@pytest.mark.parametrize("chans,roi", [(4, 16), (1, 30)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_random_affines_are_bit_exact_against_the_restatement(chans, roi, dtype):
    """+-30 degrees, zoom 0.7-1.4, with flips, quarter turns and shift / scale; rows 0-5 start at a corner of their volume"""
    vols, tens, desc = _volumes(chans)
    rng = np.random.default_rng(42)
    n = 12
    rows, picks = _rows(rng, roi, n)
    mats = np.stack([aref.random_matrix(rng) for _ in range(n)])
    got_i, got_l = _run(desc, 3, rows, picks, mats, chans, roi, dtype)
    outside = 0
    for j, (row, p) in enumerate(zip(rows, picks)):
        img, lab = vols[row.vol]
        wi, wl = aref.affine_crop(img, lab, p[3:6], roi, row.flips, row.rotk, row.shift, row.scale, mats[j], PAD)
        want = torch.from_numpy(wi).to(dtype)                                        # bf16: the fp32 result rounded once
        assert torch.equal(_bits(got_i[j].cpu()), _bits(want)), j
        assert np.array_equal(got_l[j, 0].cpu().numpy(), wl), j
        c = aref.source_coords(p[3:6], roi, row.flips, row.rotk, mats[j])
        outside += int((c.min() < -1.0) or any(c[a].max() > img.shape[1 + a] for a in range(3)))
    assert outside >= 3                                                              # whole taps outside the volume were read as pad


def test_exact_quarter_turn_matrices_equal_rot90_of_the_crop():
    """entries 0 and +-1 on an even roi: every coordinate is an integer, the patch is a rotated copy of the crop"""
    chans, roi = 4, 16
    vols, tens, desc = _volumes(chans)
    from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow
    # M maps the patch offset d to the source offset: out[p] = crop[h + M (p - h)]
    turn_zy = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])          # out[i, j] = crop[n-1-j, i]
    turn_yx = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    cases = [(turn_zy, 3, (0, 1)), (turn_zy.T, 1, (0, 1)), (turn_yx, 3, (1, 2)), (turn_yx.T, 1, (1, 2)), (turn_zy @ turn_zy, 2, (0, 1))]
    start = (9, 3, 11)
    rows = [PickRow(0, PICK_VOXEL, 0, 0, 0, 0, 0.0, 1.0)] * len(cases)
    picks = [[s + roi // 2 for s in start] + list(start) + [0, 0]] * len(cases)
    got_i, got_l = _run(desc, 3, rows, picks, np.stack([c[0] for c in cases]), chans, roi, torch.float32)
    img, lab = vols[0]
    ci = img[:, start[0]:start[0] + roi, start[1]:start[1] + roi, start[2]:start[2] + roi]
    cl = lab[start[0]:start[0] + roi, start[1]:start[1] + roi, start[2]:start[2] + roi]
    for j, (_, k, axes) in enumerate(cases):
        assert np.array_equal(got_i[j].cpu().numpy(), np.rot90(ci, k, axes=(axes[0] + 1, axes[1] + 1))), j
        assert np.array_equal(got_l[j, 0].cpu().numpy(), np.rot90(cl, k, axes=axes).astype(np.float32)), j


@pytest.mark.parametrize("roi", [16, 15])
def test_half_scale_matrix_gives_the_exact_mean_chain_of_integer_data(roi):
    """M = 0.5 I on integer-valued data.  Even roi: d = p - h is a half-integer, so every coordinate has the exact fraction
    0.25 or 0.75.  Odd roi: d is an integer, every other coordinate sits exactly on a half-integer (fraction 0.5, the label's
    floor(c + 0.5) rounds it up), the rest on voxels.  Either way the weights are exact in fp32 and the weighted mean of the 8
    neighbours, computed here per axis in float64, is what the lerp chain must give, bit for bit."""
    from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow
    chans = 4
    vols, tens, desc = _volumes(chans, integer=True)
    start = (7, 2, 12)
    img, lab = vols[1]
    rows = [PickRow(1, PICK_VOXEL, 0, 0, 0, 0, 0.0, 1.0)]
    picks = [[s + roi // 2 for s in start] + list(start) + [0, 0]]
    got_i, got_l = _run(desc, 3, rows, picks, 0.5 * np.eye(3), chans, roi, torch.float32, pad=-3.0)
    h = (roi - 1) / 2.0
    want, near = img.astype(np.float64), []
    for a in range(3):
        c = (start[a] + h) + 0.5 * (np.arange(roi) - h)                             # exact: multiples of 0.25
        i = np.floor(c).astype(int)
        f = c - i
        assert set(np.unique(f)) == ({0.25, 0.75} if roi % 2 == 0 else {0.0, 0.5})
        assert i.min() >= 0 and i.max() + 1 < img.shape[1 + a]                        # interior: no pad tap
        w = np.zeros((roi, img.shape[1 + a]))
        w[np.arange(roi), i] = 1.0 - f
        w[np.arange(roi), i + 1] = f
        want = np.moveaxis(np.tensordot(w, want, axes=(1, 1 + a)), 0, 1 + a)
        near.append(np.floor(c + 0.5).astype(int))
    assert np.array_equal(got_i[0].cpu().numpy().astype(np.float64), want)
    assert np.array_equal(got_l[0, 0].cpu().numpy(), lab[np.ix_(*near)].astype(np.float32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_double_scale_matrix_at_a_corner_pads_the_outer_shell(dtype):
    """M = 2 I reads twice the patch's extent around its centre: with roi 30 in volumes of at most 41 voxels per side the
    outermost layer of every patch lies wholly outside, whichever corner the crop starts at"""
    from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow
    chans, roi = 1, 30
    vols, tens, desc = _volumes(chans)
    rows, picks = [], []
    for vi, shape in enumerate(SHAPES):
        for start in ([0, 0, 0], [s - roi for s in shape]):
            rows.append(PickRow(vi, PICK_VOXEL, 0, 0, 0, 0, 0.0, 1.0))
            picks.append([s + roi // 2 for s in start] + start + [0, 0])
    got_i, got_l = _run(desc, 3, rows, picks, np.tile(2.0 * np.eye(3), (len(rows), 1, 1)), chans, roi, dtype)
    shell = torch.ones(roi, roi, roi, dtype=torch.bool)
    shell[1:-1, 1:-1, 1:-1] = False
    pad = torch.tensor(PAD, dtype=torch.float32).to(dtype)
    for j in range(len(rows)):
        assert bool((got_i[j, 0].cpu()[shell] == pad).all()) and bool((got_l[j, 0].cpu()[shell] == 0).all()), j
        assert bool((got_i[j, 0].cpu()[~shell] != pad).any()), j
    assert float(got_l[:4].max()) > 0                                                # the labelled volumes' interiors are read


def test_centre_voxel_is_the_source_voxel_for_any_matrix():
    """odd roi, un-flipped: d = 0 at the centre, so c = start + h exactly whatever M holds"""
    from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow
    chans, roi = 4, 15
    vols, tens, desc = _volumes(chans)
    rng = np.random.default_rng(43)
    n = 9
    rows, picks, mats = [], [], []
    for i in range(n):
        vi = i % 3
        start = [int(rng.integers(0, s - roi + 1)) for s in SHAPES[vi]]
        rows.append(PickRow(vi, PICK_VOXEL, 0, 0, 0, 0, 0.03, 1.07))
        picks.append([s + roi // 2 for s in start] + start + [0, 0])
        mats.append(rng.uniform(-3.0, 3.0, (3, 3)) if i % 3 else aref.random_matrix(rng))
    got_i, got_l = _run(desc, 3, rows, picks, np.stack(mats), chans, roi, torch.float32)
    h = roi // 2
    for j, (row, p) in enumerate(zip(rows, picks)):
        img, lab = vols[row.vol]
        src = img[:, p[3] + h, p[4] + h, p[5] + h]
        want = (src + np.float32(0.03)).astype(np.float32) * np.float32(1.07)
        assert np.array_equal(got_i[j, :, h, h, h].cpu().numpy(), want), j
        assert float(got_l[j, 0, h, h, h]) == (float(lab[p[3] + h, p[4] + h, p[5] + h]) if lab is not None else 0.0), j


def test_invalid_rows_give_zero_patches():
    """rows that name no volume or a volume with another channel count: nothing is read, the patch is all zero, the other
    rows of the batch are untouched"""
    from medicalsemseg_amd.data_device import PICK_VOXEL, PickRow
    chans, roi = 4, 16
    vols, tens, desc = _volumes(chans)
    _, _, desc1 = _volumes(1)
    rng = np.random.default_rng(44)
    ids = [0, -1, 3, 1, -7, 2]
    rows = [PickRow(v, PICK_VOXEL, 0, 0, 5, 1, 0.05, 1.1) for v in ids]
    picks = [[12, 12, 12, 4, 4, 4, 0, 0]] * len(ids)
    mats = np.stack([aref.random_matrix(rng) for _ in ids])
    for dtype in (torch.float32, torch.bfloat16):
        got_i, got_l = _run(desc, 3, rows, picks, mats, chans, roi, dtype)
        for j, v in enumerate(ids):
            if 0 <= v < 3:
                wi, wl = aref.affine_crop(vols[v][0], vols[v][1], (4, 4, 4), roi, 5, 1, 0.05, 1.1, mats[j], PAD)
                assert torch.equal(got_i[j].cpu(), torch.from_numpy(wi).to(dtype)) and np.array_equal(got_l[j, 0].cpu().numpy(), wl)
            else:
                assert float(got_i[j].float().abs().max()) == 0.0 and float(got_l[j].abs().max()) == 0.0, (j, v)
        # one-channel volumes asked for four channels: every row is a channel mismatch
        got_i, got_l = _run(desc1, 3, rows, picks, mats, chans, roi, dtype)
        assert float(got_i.float().abs().max()) == 0.0 and float(got_l.abs().max()) == 0.0


# ---- loaders --------------------------------------------------------------------------------------------------------
def _records(dev):
    """two labelled volumes as records of preprocess_volume (the loader needs a label map for its crop centres)"""
    vols, tens, _ = _volumes(1)
    return [{"img": tens[k][0], "lab": tens[k][1], "affine": np.eye(4), "original_affine": np.eye(4), "filename": f"/data/v{k}.nii.gz"}
            for k in range(2)], vols


def _collect(loader, check=None):
    out = []
    for b in loader:
        out.append((b["image"].clone(), b["label"].clone()))
        if check:
            check(loader, b)
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("crop", ["fgbg", "spatial"])
def test_device_dataset_loader_with_affine(crop):
    from medicalsemseg_amd.data_device import DeviceDatasetLoader
    dev = _dev()
    recs, vols = _records(dev)
    roi, ppi, batch, n_batches = 16, 2, 4, 3
    kw = dict(patches_per_image=ppi, device=dev, seed=23, crop=crop, pos=2.0, neg=1.0, flip_prob=0.5, rot_prob=0.6,
              shift_prob=0.5, scale_prob=0.5, image_threshold=0.0)
    seen = []

    def check(ld, b):
        assert ld.last_mats.shape == (batch, 3, 3) and ld.last_mats.dtype == np.float64
        for j, row in enumerate(ld.last_rows):
            img, lab = vols[row.vol]
            wi, wl = aref.affine_crop(img, lab, [int(v) for v in ld.last_picks[j, 3:6]], roi, row.flips, row.rotk, row.shift,
                                      row.scale, ld.last_mats[j], PAD)
            assert np.array_equal(b["image"][j].cpu().numpy(), wi) and np.array_equal(b["label"][j, 0].cpu().numpy(), wl), j
            seen.append(not np.array_equal(ld.last_mats[j], np.eye(3)))
            cen = [float(c[j]) for c in b["image_transforms"][0]["extra_info"]["center"]]
            assert cen == [float(v) for v in ld.last_picks[j, :3]]                   # the recorded centre is the patch centre

    a = DeviceDatasetLoader(recs, roi, batch, n_batches, affine_prob=1.0, affine_pad=PAD, **kw)
    b = DeviceDatasetLoader(recs, roi, batch, n_batches, affine_prob=1.0, affine_pad=PAD, **kw)
    ba, bb = _collect(a, check), _collect(b)
    assert _same(ba, bb) and a.launches == n_batches == len(ba) and all(seen)
    seen.clear()
    half = DeviceDatasetLoader(recs, roi, batch, n_batches, affine_prob=0.5, affine_rotate=(30.0, 0.0, 10.0), affine_zoom=(0.9, 1.1),
                               affine_pad=PAD, **kw)
    _collect(half, check)
    assert any(seen) and not all(seen) and half.launches == n_batches
    # probability 0: the batches of a loader built without the new arguments, from the same kernels
    zero = DeviceDatasetLoader(recs, roi, batch, n_batches, affine_prob=0.0, **kw)
    plain = DeviceDatasetLoader(recs, roi, batch, n_batches, **kw)
    assert _same(_collect(zero), _collect(plain)) and zero.last_mats is None and not _same(ba, _collect(plain))


def test_device_patch_loader_with_affine():
    from medicalsemseg_amd.data_device import DevicePatchLoader
    dev = _dev()
    vols, tens, _ = _volumes(4)
    img, lab = vols[0]
    roi, batch, n_batches = 16, 3, 3
    kw = dict(seed=24, pos=2.0, neg=1.0, flip_prob=0.5, rot_prob=0.6, shift_prob=0.5, scale_prob=0.5)
    seen = []

    def check(ld, b):
        for j, row in enumerate(ld.last_rows):
            assert [int(v) for v in ld.last_picks[j, 3:6]] == [row.z0, row.y0, row.x0]
            wi, wl = aref.affine_crop(img, lab, (row.z0, row.y0, row.x0), roi, row.flips, row.rotk, row.shift, row.scale,
                                      ld.last_mats[j], 0.25)
            assert np.array_equal(b["image"][j].cpu().numpy(), wi) and np.array_equal(b["label"][j, 0].cpu().numpy(), wl), j
            seen.append(not np.array_equal(ld.last_mats[j], np.eye(3)))

    mk = lambda **extra: DevicePatchLoader(torch.from_numpy(img), torch.from_numpy(lab), roi, batch, n_batches, dev, **kw, **extra)
    a, b = mk(affine_prob=1.0, affine_pad=0.25), mk(affine_prob=1.0, affine_pad=0.25)
    ba, bb = _collect(a, check), _collect(b)
    assert _same(ba, bb) and a.launches == n_batches and all(seen)
    seen.clear()
    _collect(mk(affine_prob=0.5, affine_pad=0.25), check)
    assert any(seen) and not all(seen)
    zero, plain = mk(affine_prob=0.0), mk()
    assert _same(_collect(zero), _collect(plain)) and zero.last_mats is None and not _same(ba, _collect(plain))


# ---- the training driver end to end -----------------------------------------------------------------------------------
def _finite_losses(out_dir, n):
    log = [json.loads(l) for l in open(os.path.join(out_dir, "log.txt"))]
    assert len(log) == n and all(np.isfinite(e["train/loss"]) for e in log), log


def test_run_training_synthetic_with_affine(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "run_training.py"), "--synthetic", "--model", "UNetSmall", "--output_dim", "2",
           "--vol_size", "32", "--n_images_per_batch", "2", "--synthetic_steps", "2", "--epochs", "1", "--val_interval", "1",
           "--synthetic_val_size", "48", "--warmup_epochs", "0", "--output_dir", str(tmp_path), "--t_rand_crop_fgbg",
           "--t_flip_prob", "0.5", "--t_rot_prob", "0.5", "--t_affine_prob", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _finite_losses(str(tmp_path), 1)


def test_run_training_on_files_with_affine(tmp_path):
    from tests import dataprep_ref as ref
    ref.write_ct_dataset(str(tmp_path / "data" / "Task99_CT"), n=6, n_cls=2)
    out = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "run_training.py"), "--model", "UNetSmall", "--output_dim", "2", "--vol_size", "32",
           "--t_voxel_spacings", "--t_voxel_dims", "1.0", "1.0", "1.0", "--t_fixed_ct_intensity", "--t_crop_foreground_img",
           "--t_spatial_pad", "--t_normalize", "--t_rand_crop_fgbg", "--t_n_patches_per_image", "2", "--t_flip_prob", "0.5",
           "--t_rot_prob", "0.5", "--n_images_per_batch", "2", "--json_list", "dataset.json", "--task", "Task99_CT", "--data_path",
           str(tmp_path / "data"), "--epochs", "1", "--val_interval", "1", "--warmup_epochs", "0", "--output_dir", out,
           "--t_affine_prob", "0.5", "--t_affine_rotate", "30", "10", "10", "--t_affine_zoom", "0.8", "1.25"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _finite_losses(out, 1)
