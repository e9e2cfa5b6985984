"""Class-ratio crop centres on the GPU without a dilation: msseg_class_slab_counts, msseg_class_pick_voxels and
DeviceDatasetLoader(crop="class_ratios") against the restatement of tests/class_crop_ref.py.  Everything is exact."""
import numpy as np
import pytest
import torch

from tests import class_crop_ref as ref

pytestmark = pytest.mark.gpu

THR = 0.25


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _volume(shape, values, seed, chans=1):
    """image with a tenth of its voxels exactly on the threshold (they separate "gt" from "ne"), labels from `values`"""
    rng = np.random.default_rng(seed)
    img = rng.standard_normal((chans,) + shape).astype(np.float32)
    img[0][rng.random(shape) < 0.1] = np.float32(THR)
    lab = rng.choice(np.array(values, dtype=np.uint8), size=shape)
    return img, lab


def _gpu(img, lab):
    dev = _dev()
    return torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)


def _desc(pairs):
    from medicalsemseg_amd.data_device import VolumeDesc, _upload
    return _upload([VolumeDesc(i.data_ptr(), l.data_ptr(), *i.shape) for i, l in pairs], _dev())


def _pick(desc, nvol, rows, roi, rule, masks=None):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import _upload
    out = torch.empty(len(rows), 8, dtype=torch.int32, device=_dev())
    hip.class_pick_voxels(desc, nvol, _upload(rows, _dev()), len(rows), roi, THR, out, rule, masks=masks)
    return out.cpu().numpy()


def _all_rank_rows(cands, vol=0):
    """for every class and slice the ranks 0 .. count (the last one is beyond the count) -> (rows, expected in-slice index)"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import PickRow
    rows, want = [], []
    for c, cand in enumerate(cands):
        for z in range(cand.shape[0]):
            for k in range(int(cand[z].sum()) + 1):
                rows.append(PickRow(vol, hip.PICK_CLASS0 + c, z, k, 0, 0, 0.0, 1.0))
                want.append((z, ref.kth_in_slice(cand, z, k)))
    return rows, want


@pytest.fixture(scope="module")
def chunky():
    """[5, 37, 70]: H * W = 2590 is more than one 2048-voxel scan chunk and W is no multiple of 8.  Values {0, 1, 3, 4} with
    K = 3: class 2 is absent from the volume, 3 and 4 belong to no class; class 1 is absent from slice 2; slice 1 holds class
    1 at the in-slice flat indices 2047 and 2048 (the chunk border) with an image value that passes both rules."""
    shape = (5, 37, 70)
    img, lab = _volume(shape, (0, 1, 3, 4), 31)
    lab[2][lab[2] == 1] = 0
    for flat in (2047, 2048):
        lab[1].reshape(-1)[flat] = 1
        img[0, 1].reshape(-1)[flat] = 1.0
    return img, lab


@pytest.mark.parametrize("rule", ["gt", "ne"])
def test_counts_and_every_rank_on_a_slice_of_more_than_one_chunk(chunky, rule):
    from medicalsemseg_amd import hip
    img, lab = chunky
    K, roi = 3, 16
    ti, tl = _gpu(img, lab)
    got = hip.class_slab_counts(ti, tl, K, THR, rule)
    want = ref.slab_counts(img[0], lab, K, 0, THR, rule)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert want[2, 1] == 0 and want[:, 2].sum() == 0 and want[:, 0].min() > 0 and want[1, 1] > 2
    # the image rule bites on every class, and the two rules differ
    assert want.sum() < (lab < K).sum() and not np.array_equal(want, ref.slab_counts(img[0], lab, K, 0, THR, "ne" if rule == "gt" else "gt"))
    cands = [ref.candidates(img[0], lab, c, 0, THR, rule) for c in range(K)]
    rows, expect = _all_rank_rows(cands)
    assert len(rows) == int(want.sum()) + 5 * K
    out = _pick(_desc([(ti, tl)]), 1, rows, roi, rule)
    hits = set()
    for row, (z, hit), o in zip(rows, expect, out):
        assert o.tolist() == ref.pick_row(lab.shape, z, hit, roi), (row.mode, z, row.rank)
        hits.add((z, hit))
    assert (1, 2047) in hits and (1, 2048) in hits and (2, -1) in hits


def test_sixteen_classes():
    from medicalsemseg_amd import hip
    shape, K = (3, 9, 11), 16
    img, lab = _volume(shape, tuple(range(18)), 32)
    ti, tl = _gpu(img, lab)
    want = ref.slab_counts(img[0], lab, K, 0, THR)
    assert np.array_equal(hip.class_slab_counts(ti, tl, K, THR).cpu().numpy(), want) and (want.sum(0) > 0).all()
    cands = [ref.candidates(img[0], lab, c, 0, THR) for c in range(K)]
    rows, expect = _all_rank_rows(cands)
    out = _pick(_desc([(ti, tl)]), 1, rows, 4, "gt")
    for (z, hit), o in zip(expect, out):
        assert o.tolist() == ref.pick_row(shape, z, hit, 4)
    with pytest.raises(ValueError):
        hip.class_slab_counts(ti, tl, 17, THR)
    with pytest.raises(ValueError):
        hip.class_slab_counts(ti, tl, 0, THR)


@pytest.mark.parametrize("rule", ["gt", "ne"])
def test_class_zero_of_two_classes_is_the_background_pick_and_old_modes_pass_through(rule):
    """K = 2: lab == 0 with the image rule is the background candidate set, so class-0 rows give the rows PICK_BG gives,
    bit for bit; rows of mode 0 / 1 / 2 through the new entry point equal msseg_pick_voxels"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import PICK_BG, PICK_FG, PICK_VOXEL, PickRow, _upload
    dev = _dev()
    shape, roi = (6, 37, 70), 16
    img, lab = _volume(shape, (0, 0, 1), 33)
    ti, tl = _gpu(img, lab)
    desc = _desc([(ti, tl)])
    counts = hip.slab_counts(ti, tl, THR, rule).cpu().numpy()                        # [D, 2] = fg, bg
    cls = hip.class_slab_counts(ti, tl, 2, THR, rule).cpu().numpy()
    assert np.array_equal(cls[:, 0], counts[:, 1])
    old_rows, new_rows = [], []
    for z in range(shape[0]):
        n = int(counts[z, 1])
        for k in sorted({0, 1, 7, n // 3, n // 2, n - 2, n - 1, n, n + 5}):
            old_rows.append(PickRow(0, PICK_BG, z, k, 0, 0, 0.0, 1.0))
            new_rows.append(PickRow(0, hip.PICK_CLASS0, z, k, 0, 0, 0.0, 1.0))
    for z in (-1, 0, 3, 5, 9):                                                        # z outside the volume is clamped
        for mode, k in ((PICK_FG, 0), (PICK_FG, 11), (PICK_FG, 10 ** 6), (PICK_BG, 3), (PICK_VOXEL, 2589), (PICK_VOXEL, -4),
                        (PICK_VOXEL, 10 ** 6)):
            old_rows.append(PickRow(0, mode, z, k, 0, 0, 0.0, 1.0))
            new_rows.append(PickRow(0, mode, z, k, 0, 0, 0.0, 1.0))
    old_rows.append(PickRow(3, PICK_BG, 0, 0, 0, 0, 0.0, 1.0))                       # a row that names no volume
    new_rows.append(PickRow(3, hip.PICK_CLASS0, 0, 0, 0, 0, 0.0, 1.0))
    old = torch.empty(len(old_rows), 8, dtype=torch.int32, device=dev)
    hip.pick_voxels(desc, 1, _upload(old_rows, dev), len(old_rows), roi, THR, old, rule)
    new = _pick(desc, 1, new_rows, roi, rule)
    assert np.array_equal(old.cpu().numpy(), new)
    assert (new[:, 7] >= 0).sum() > 40 and (new[:, 7] == -1).sum() >= 12
    # a mode that names neither an old pick nor a class reports no candidate
    odd = _pick(desc, 1, [PickRow(0, m, 2, 0, 0, 0, 0.0, 1.0) for m in (3, 15, 32, -1)], roi, rule)
    assert (odd[:, 7] == -1).all() and (odd[:, 6] == 2).all()


def _records(vols, dev):
    out = []
    for k, (img, lab) in enumerate(vols):
        aff = np.eye(4)
        aff[0, 0] = 1.0 + k
        out.append({"img": torch.from_numpy(img).to(dev), "lab": torch.from_numpy(lab).to(dev), "affine": aff,
                    "original_affine": aff + 1.0, "filename": f"vol{k}.nii.gz"})
    return out


def test_loader_draws_only_the_class_asked_for_and_gathers_its_crop():
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import DeviceDatasetLoader
    from medicalsemseg_amd.utils import misc
    dev = _dev()
    roi, batch = 16, 6
    vols = [_volume(s, (0, 0, 0, 1, 2, 3), 40 + k, chans=2) for k, s in enumerate([(20, 37, 70), (33, 18, 25), (17, 40, 19)])]
    ld = DeviceDatasetLoader(_records(vols, dev), roi, batch, 4, patches_per_image=2, device=dev, seed=5, crop="class_ratios",
                             class_ratios=(0.0, 0.0, 1.0), image_threshold=THR)
    want_counts = [ref.slab_counts(i[0], l, 3, 0, THR).sum(0).tolist() for i, l in vols]
    assert ld.class_candidates == want_counts and ld.masks == [] and ld.mask_ptrs is None
    seen = set()
    for b in ld:
        assert ld.last_classes == [2] * batch and all(r.mode == hip.PICK_CLASS0 + 2 for r in ld.last_rows)
        tr = b["image_transforms"][0]
        assert tr["class"] == ["RandCropByClassesd"] * batch
        rel = misc.get_rel_crop_loc(tr)
        assert tuple(rel.shape) == (batch, 3) and float(rel.min()) > 0 and float(rel.max()) < 1
        cen = torch.stack(tr["extra_info"]["center"], 1)
        for j, (row, p) in enumerate(zip(ld.last_rows, ld.last_picks.tolist())):
            img, lab = vols[row.vol]
            D, H, W = lab.shape
            z, yx = p[6], p[7]
            assert yx >= 0 and lab[z, yx // W, yx % W] == 2 and img[0, z, yx // W, yx % W] > THR
            assert p == ref.pick_row(lab.shape, z, yx, roi) and cen[j].tolist() == [float(v) for v in p[:3]]
            z0, y0, x0 = p[3:6]
            assert np.array_equal(b["image"][j].cpu().numpy(), img[:, z0:z0 + roi, y0:y0 + roi, x0:x0 + roi])
            assert np.array_equal(b["label"][j, 0].cpu().numpy(), lab[z0:z0 + roi, y0:y0 + roi, x0:x0 + roi].astype(np.float32))
            assert b["image_meta_dict"]["filename_or_obj"][j] == f"vol{row.vol}.nii.gz"
            seen.add(row.vol)
    assert seen == {0, 1, 2} and ld.launches == 4
    # seeded: a second loader repeats the picks
    again = DeviceDatasetLoader(_records(vols, dev), roi, batch, 4, patches_per_image=2, device=dev, seed=5, crop="class_ratios",
                                class_ratios=(0.0, 0.0, 1.0), image_threshold=THR)
    for _ in again:
        pass
    assert torch.equal(again.last_picks, ld.last_picks)


def test_loader_never_draws_a_class_the_volume_lacks_and_falls_back_without_candidates():
    from medicalsemseg_amd.data_device import PICK_VOXEL, DeviceDatasetLoader
    dev = _dev()
    img, lab = _volume((18, 21, 33), (0, 1, 1), 50)
    ld = DeviceDatasetLoader(_records([(img, lab)], dev), 16, 8, 8, device=dev, seed=6, crop="class_ratios",
                             class_ratios=(1.0, 1.0, 1.0), image_threshold=THR, flip_prob=0.5, rot_prob=0.5)
    assert ld.class_candidates[0][2] == 0 and min(ld.class_candidates[0][:2]) > 0
    classes = []
    for _ in ld:
        classes += ld.last_classes
        for c, p in zip(ld.last_classes, ld.last_picks.tolist()):
            assert lab[p[6], p[7] // 33, p[7] % 33] == c
    assert set(classes) == {0, 1}
    # no voxel passes the image rule: no candidate of any class, a uniform voxel of the volume
    none = DeviceDatasetLoader(_records([(img, lab)], dev), 16, 4, 2, device=dev, seed=6, crop="class_ratios",
                               class_ratios=(1.0, 1.0, 1.0), image_threshold=1e9)
    assert none.class_candidates == [[0, 0, 0]]
    for b in none:
        assert none.last_classes == [-1] * 4 and all(r.mode == PICK_VOXEL for r in none.last_rows)
        assert (none.last_picks[:, 7] >= 0).all() and tuple(b["image"].shape) == (4, 1, 16, 16, 16)


def test_run_training_synthetic_with_class_ratios(tmp_path):
    """the driver end to end without files: the synthetic volume in a cache record, crops by class, candidates reported"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "run_training.py"), "--synthetic", "--model", "UNetSmall", "--output_dim", "3",
           "--vol_size", "32", "--n_images_per_batch", "2", "--synthetic_steps", "2", "--epochs", "2", "--val_interval", "2",
           "--synthetic_val_size", "32", "--warmup_epochs", "1", "--output_dir", str(tmp_path), "--t_flip_prob", "0.5",
           "--t_rand_crop_class_ratios", "0", "1", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "synthetic_volume crop-centre candidates per class (ratios [0.0, 1.0, 2.0], dilation 0): [" in r.stdout
    assert os.path.exists(os.path.join(str(tmp_path), "log.txt"))
    r = subprocess.run(cmd + ["--t_rand_crop_fgbg"], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode != 0 and "--t_rand_crop_class_ratios" in r.stderr and "--t_rand_crop_fgbg" in r.stderr


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    from medicalsemseg_amd import hip
    img, lab = _volume((4, 5, 6), (0, 1), 60)
    ti, tl = _gpu(img, lab)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.class_slab_counts(torch.from_numpy(img), torch.from_numpy(lab), 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.class_slab_counts(ti, torch.from_numpy(lab), 2)
    with pytest.raises(AssertionError):
        hip.class_slab_counts(ti.double(), tl, 2)
    with pytest.raises(AssertionError):
        hip.class_slab_counts(ti, tl.int(), 2)
    with pytest.raises(AssertionError):
        hip.class_slab_counts(ti, tl[:, :, :5], 2)
    with pytest.raises(AssertionError):
        hip.class_slab_counts(ti, tl, 2, mask=tl)
    desc = _desc([(ti, tl)])
    rows = torch.zeros(32, dtype=torch.uint8, device=_dev())
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.class_pick_voxels(desc, 1, rows, 1, 4, 0.0, torch.empty(1, 8, dtype=torch.int32))
    with pytest.raises(AssertionError):
        hip.class_pick_voxels(desc, 1, rows, 1, 4, 0.0, torch.empty(1, 8, dtype=torch.int64, device=_dev()))
    with pytest.raises(AssertionError):
        hip.class_pick_voxels(desc, 1, rows, 1, 4, 0.0, torch.empty(1, 8, dtype=torch.int32, device=_dev()),
                              masks=torch.zeros(1, dtype=torch.int32, device=_dev()))
