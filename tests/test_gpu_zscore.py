"""Per-volume z-score over the non-zero voxels on the GPU (csrc/volume_stats.hip, --t_zscore / --t_zscore_clip) against the
numpy restatement of tests/zscore_ref.py, the `!=` background rule of the crop-centre pick, and preprocess_volume with the
flags on a 2-channel 4-D NIfTI.

Shapes: [2, 21, 19, 37] (W neither a multiple of 4 nor of 64; an odd channel size, so channel 1 starts off a 16-byte
boundary), [1, 8, 8, 300] (crosses a 256-thread block along x), [3, 70, 70, 70] (many blocks per channel: partial rows and
the cross-block histogram flush)."""
import os

import numpy as np
import pytest
import torch

from tests import dataprep_ref as ref
from tests import zscore_ref as zr

pytestmark = pytest.mark.gpu

SHAPES = [(2, 21, 19, 37), (1, 8, 8, 300), (3, 70, 70, 70)]
CLIP = (0.5, 99.5)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _channel(kind, shape, rng):
    """one float32 channel.  mixed: both signs, a fifth of the voxels +-0.0, a quarter equal to one value (ties through every
    radix pass); offset: |mean| / std = 1e3; constant: one non-zero value and zeros; single: one non-zero voxel; empty"""
    n = int(np.prod(shape))
    if kind == "empty":
        return np.zeros(shape, np.float32)
    if kind == "single":
        v = np.zeros(n, np.float32)
        v[n // 3] = -2.5
        return v.reshape(shape)
    if kind == "constant":
        v = np.full(n, 3.25, np.float32)
        v[rng.random(n) < 0.4] = 0.0
        return v.reshape(shape)
    if kind == "offset":
        v = (1000.0 + rng.standard_normal(n)).astype(np.float32)
        v[rng.random(n) < 0.3] = 0.0
        return v.reshape(shape)
    assert kind == "mixed"
    v = (rng.standard_normal(n) * 50.0 + 20.0).astype(np.float32)
    u = rng.random(n)
    v[u < 0.25] = np.float32(1.5)
    v[(u >= 0.25) & (u < 0.35)] = 0.0
    v[(u >= 0.35) & (u < 0.45)] = -0.0
    return v.reshape(shape)


ORDER_KINDS = {2: ("mixed", "empty"), 1: ("mixed",), 3: ("mixed", "single", "empty")}
MOMENT_KINDS = {2: ("mixed", "offset"), 1: ("offset",), 3: ("constant", "mixed", "offset")}


def _volume(shape, kinds, seed):
    rng = np.random.default_rng(seed)
    return np.stack([_channel(k, shape[1:], rng) for k in kinds])


@pytest.mark.parametrize("shape", SHAPES)
def test_order_statistics_are_bit_exact(shape):
    from medicalsemseg_amd import hip
    x = _volume(shape, ORDER_KINDS[shape[0]], 31)
    assert np.signbit(x[0][x[0] == 0]).any() and not np.signbit(x[0][x[0] == 0]).all() and (x[0] < 0).any() and (x[0] > 0).any()
    xd = torch.from_numpy(x).to(_dev())
    srt = [np.sort(c[c != 0]) for c in x]

    def check(out, ranks_per_channel):
        out = out.cpu().numpy()
        for c, (s, ranks) in enumerate(zip(srt, ranks_per_channel)):
            assert out[c, 0] == s.size
            for j, k in enumerate(ranks):
                if k < s.size:
                    assert out[c, 1 + j] == s[k], (c, j, k, out[c, 1 + j], s[k])       # ==: -0.0 and 0.0 are not told apart
                else:
                    assert np.isnan(out[c, 1 + j]), (c, j, k)
            assert all(np.isnan(v) for v in out[c, 1 + len(ranks):5])
        return out

    # explicit ranks: the first, one inside, the last of channel 0, one past every channel's end
    n0 = srt[0].size
    ranks = (0, 5, n0 - 1, n0 + 10 ** 6)
    out = check(hip.select_f32(xd, ranks=ranks), [ranks] * shape[0])
    assert (out[:, 5] == -np.inf).all() and (out[:, 6] == np.inf).all()
    # percentages: (0, 100) asks for ranks 0, 1 and n - 1 twice (the clamped k + 1); CLIP for its four ranks
    for pct in ((0.0, 100.0), CLIP):
        want_ranks = []
        for s in srt:
            n = s.size
            want_ranks.append([r for q in pct for r in zr.ranks_of(q, n)[:2]] if n else [0, 1, 0, 1])
        out = check(hip.select_f32(xd, percentages=pct), want_ranks)
        for c, s in enumerate(srt):
            if s.size:
                assert out[c, 5] == zr.percentile_f32(s, pct[0]) and out[c, 6] == zr.percentile_f32(s, pct[1])
            else:
                assert out[c, 5] == -np.inf and out[c, 6] == np.inf
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))              # the select only reads


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("clip", [None, CLIP])
def test_moments_against_the_float64_restatement(shape, clip):
    """mean and std to 1e-10 relative: a double sum of <= 2^20 fp32 terms is off by at most n 2^-53 = 1.2e-10 relative to
    the sum of the magnitudes, and the second pass over the deviations removes the cancellation of E[y^2] - mean^2"""
    from medicalsemseg_amd import hip
    kinds = MOMENT_KINDS[shape[0]]
    x = _volume(shape, kinds, 32)
    xd = torch.from_numpy(x).to(_dev())
    bounds = None
    if clip is not None:
        bounds = hip.select_f32(xd, percentages=clip)[:, 5:7]
    a = hip.masked_moments(xd, bounds)
    b = hip.masked_moments(xd, bounds)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))                             # bit-identical from run to run
    got = a.cpu().numpy()
    for c, kind in enumerate(kinds):
        n, lo, hi, mean, std = zr.channel_stats(x[c], clip)
        print(f"{shape} {kind} clip {clip}: n {got[c, 0]:.0f} mean {got[c, 3]!r} (want {mean!r}) std {got[c, 4]!r} (want {std!r})")
        assert got[c, 0] == n and got[c, 1] == lo and got[c, 2] == hi and got[c, 5] == 0
        assert abs(got[c, 3] - mean) <= 1e-10 * abs(mean) and abs(got[c, 4] - std) <= 1e-10 * std
        if kind == "constant":
            assert got[c, 3] == 3.25 and got[c, 4] == 1.0                                     # std 0 -> 1
        if kind == "offset":
            assert abs(mean) / std > 900.0


def test_moments_of_empty_and_single_voxel_channels():
    from medicalsemseg_amd import hip
    x = _volume((3, 5, 7, 9), ("empty", "single", "mixed"), 33)
    got = hip.masked_moments(torch.from_numpy(x).to(_dev())).cpu().numpy()
    assert got[0].tolist() == [0.0, -np.inf, np.inf, 0.0, 1.0, 0.0]
    assert got[1].tolist() == [1.0, -np.inf, np.inf, -2.5, 1.0, 0.0]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("clip", [None, CLIP])
def test_apply_bit_exact_and_end_to_end(shape, clip):
    from medicalsemseg_amd import hip
    kinds = ("mixed", "offset", "single")[:shape[0]] if shape[0] < 3 else ("mixed", "empty", "offset")
    x = _volume(shape, kinds, 34)
    xd = torch.from_numpy(x).to(_dev())
    stats = hip.zscore_nonzero_(xd, clip)
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (shape[0], 6) and stats.is_cuda
    st, got = stats.cpu().numpy(), xd.cpu().numpy()
    # step 4 of the restatement with the statistics the device reported: every bit, the voxels outside the mask included
    for c in range(shape[0]):
        want = zr.apply_channel(x[c], *st[c, 1:5])
        assert np.array_equal(got[c].view(np.uint32), want.view(np.uint32)), (c, kinds[c])
        assert np.array_equal(got[c][x[c] == 0].view(np.uint32), x[c][x[c] == 0].view(np.uint32))
    # against the restatement alone: 1 ulp in each of mean, std and the bounds
    want, wst = zr.zscore_nonzero(x, clip)
    assert np.array_equal(st[:, 0], wst[:, 0]) and (st[:, 5] == 0).all()
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6)
    if clip is None:
        assert (st[:, 1] == -np.inf).all() and (st[:, 2] == np.inf).all()


def test_wrappers_refuse_bad_arguments():
    from medicalsemseg_amd import hip
    x = torch.zeros(1, 4, 4, 4, device=_dev())
    with pytest.raises(hip.MssegError, match="percentage"):
        hip.select_f32(x, percentages=(5.0, 101.0))
    with pytest.raises(hip.MssegError, match="rank"):
        hip.select_f32(x, ranks=(0, 1, 2, 3, 4))
    with pytest.raises(hip.MssegError, match="aligned"):
        hip.masked_moments(torch.zeros(2, 3, device=_dev())[1:])                              # 12 bytes into the allocation
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.zscore_nonzero_(torch.zeros(1, 4, 4, 4))


# ---- the background-centre rule -----------------------------------------------------------------------------------------
def test_pick_rule_ne_counts_and_picks_the_nonzero_mask():
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import PICK_BG, PickRow, VolumeDesc, _upload
    dev = _dev()
    rng = np.random.default_rng(35)
    shape, roi = (20, 41, 50), 16
    img = rng.standard_normal((1,) + shape).astype(np.float32)                              # in-mask values of both signs
    img[0][rng.random(shape) < 0.5] = 0.0
    img[0, :3] = 0.0                                                                         # slices without a candidate
    lab = (ref.ellipsoid_labels(shape, 3) > 1).astype(np.uint8)
    imd, lad = torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev)
    cand = (lab == 0) & (img[0] != 0)
    want_counts = np.stack([(lab > 0).reshape(shape[0], -1).sum(1), cand.reshape(shape[0], -1).sum(1)], 1).astype(np.int32)
    got = hip.slab_counts(imd, lad, 0.0, rule="ne").cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want_counts)
    assert not np.array_equal(got, ref.slab_counts(img[0], lab, 0.0))                        # "gt" sees half of them
    lst = np.nonzero(cand.reshape(-1))[0]
    cum = np.cumsum(want_counts[:, 1].astype(np.int64))
    idxs = [0, lst.size - 1] + [int(rng.integers(0, lst.size)) for _ in range(62)]
    rows = []
    for idx in idxs:
        z = int(np.searchsorted(cum, idx, side="right"))
        rows.append(PickRow(0, PICK_BG, z, idx - (int(cum[z - 1]) if z else 0), 0, 0, 0.0, 1.0))
    desc = _upload([VolumeDesc(imd.data_ptr(), lad.data_ptr(), *imd.shape)], dev)
    table = _upload(rows, dev)
    out = torch.empty(len(rows), 8, dtype=torch.int32, device=dev)
    hip.pick_voxels(desc, 1, table, len(rows), roi, 0.0, out, rule="ne")
    out = out.cpu().numpy()
    flat = out[:, 6].astype(np.int64) * shape[1] * shape[2] + out[:, 7]
    assert (out[:, 7] >= 0).all() and np.array_equal(flat, lst[idxs])
    assert (lab.reshape(-1)[flat] == 0).all() and (img[0].reshape(-1)[flat] != 0).all()
    assert (img[0].reshape(-1)[flat] < 0).any()                                              # picks "gt" cannot make
    # rule "gt", which is the default, against numpy on the same volume
    gt_c = hip.slab_counts(imd, lad, 0.0, rule="gt")
    assert np.array_equal(gt_c.cpu().numpy(), ref.slab_counts(img[0], lab, 0.0)) and torch.equal(gt_c, hip.slab_counts(imd, lad, 0.0))
    lst_gt = np.nonzero(((lab == 0) & (img[0] > 0)).reshape(-1))[0]
    cum_gt = np.cumsum(gt_c.cpu().numpy()[:, 1].astype(np.int64))
    assert cum_gt[-1] == lst_gt.size
    idxs_gt = [int(rng.integers(0, lst_gt.size)) for _ in range(64)]
    rows_gt = []
    for idx in idxs_gt:
        z = int(np.searchsorted(cum_gt, idx, side="right"))
        rows_gt.append(PickRow(0, PICK_BG, z, idx - (int(cum_gt[z - 1]) if z else 0), 0, 0, 0.0, 1.0))
    table = _upload(rows_gt, dev)
    gt_p = torch.empty(64, 8, dtype=torch.int32, device=dev)
    def_p = torch.empty(64, 8, dtype=torch.int32, device=dev)
    hip.pick_voxels(desc, 1, table, 64, roi, 0.0, gt_p, rule="gt")
    hip.pick_voxels(desc, 1, table, 64, roi, 0.0, def_p)
    assert torch.equal(gt_p, def_p) and (gt_p[:, 7] >= 0).all()
    gt_p = gt_p.cpu().numpy()
    assert np.array_equal(gt_p[:, 6].astype(np.int64) * shape[1] * shape[2] + gt_p[:, 7], lst_gt[idxs_gt])
    with pytest.raises(ValueError, match="'gt'.*'ne'"):
        hip.slab_counts(imd, lad, 0.0, rule="lt")


# ---- preprocess_volume --------------------------------------------------------------------------------------------------
ZS_FLAGS = ["--vol_size", "32", "--in_chans", "2", "--t_crop_foreground_img", "--t_spatial_pad"]


def _mr_case(tmp_path):
    """a skull-stripped two-modality blob in a zero surround, 4-D NIfTI (channels last) + label; the blob is thinner than
    the roi along the last axis"""
    from medicalsemseg_amd.utils.nifti import save_nifti
    rng = np.random.default_rng(36)
    shape = (46, 52, 30)
    ax = [np.linspace(-1, 1, s) for s in shape]
    r = np.sqrt((ax[0][:, None, None] / 0.8) ** 2 + (ax[1][None, :, None] / 0.85) ** 2 + (ax[2][None, None, :] / 0.7) ** 2)
    blob = r < 1.0
    img = np.zeros(shape + (2,), np.float32)
    img[..., 0] = np.where(blob, 500.0 + 120.0 * rng.standard_normal(shape), 0.0)
    img[..., 1] = np.where(blob, 3.0 + 0.6 * rng.standard_normal(shape), 0.0)
    img[23, 26, 15] = 0.0                                                                    # a zero inside the blob
    lab = (r < 0.4).astype(np.uint8)
    aff = np.diag([1.0, 1.0, 1.0, 1.0])
    ip, lp = str(tmp_path / "img_mr.nii.gz"), str(tmp_path / "lab_mr.nii.gz")
    save_nifti(ip, img, aff)
    save_nifti(lp, lab, aff)
    return {"image": ip, "label": lp}


def test_preprocess_volume_zscores_each_channel_last(tmp_path):
    from medicalsemseg_amd import data_files as df
    from medicalsemseg_amd.data_device import DeviceDatasetLoader, preprocess_volume, restore_geometry
    from medicalsemseg_amd.utils.arguments import get_args
    dev = _dev()
    item = _mr_case(tmp_path)
    image, label, aff = df.load_case(item)
    assert image.shape == (2, 46, 52, 30) and image.dtype == np.float32
    cfg = get_args(ZS_FLAGS + ["--t_zscore", "--t_zscore_clip", "0.5", "99.5"])
    rec = preprocess_volume(image, label, aff, cfg, dev, item["image"])
    rec0 = preprocess_volume(image, label, aff, get_args(ZS_FLAGS), dev, item["image"])
    # the restated chain: foreground box -> crop -> pad with 0 -> z-score of every channel over its non-zero voxels
    box = ref.foreground_box(image)
    cropped = ref.crop_pad(image, box, (32,) * 3, np.float32(0.0))
    inside = ref.crop_pad(np.ones_like(image), box, (32,) * 3, np.float32(0.0)) > 0
    assert cropped.shape[3] == 32 and box[5] - box[2] < 32 and not inside.all()              # padded along the last axis
    want, wst = zr.zscore_nonzero(cropped, CLIP)
    got = rec["img"].cpu().numpy()
    assert got.shape == want.shape and np.array_equal(rec0["img"].cpu().numpy(), cropped)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-6)
    assert (got[~inside] == 0).all() and not np.signbit(got[~inside]).any()                  # the pads are exactly 0
    assert (got[cropped == 0] == 0).all()                                                    # so is every other zero
    st = rec["zscore"]
    assert isinstance(st, np.ndarray) and st.shape == (2, 6) and np.array_equal(st[:, 0], wst[:, 0])
    assert np.allclose(st[:, 1:5], wst[:, 1:5], rtol=1e-6, atol=0) and st[0, 3] > 100 * st[1, 3]   # two scales
    for c in range(2):
        v = got[c][cropped[c] != 0].astype(np.float64)
        print(f"channel {c}: masked mean {v.mean():.3e}, masked std {v.std():.8f}, stats {st[c].tolist()}")
        assert abs(v.mean()) < 1e-5 and abs(v.std() - 1.0) < 1e-4
    # the geometry is that of the same call without the flag: restore_native_u8 is unaffected
    g, g0 = restore_geometry(rec), restore_geometry(rec0)
    assert g.keys() == g0.keys() and all(np.array_equal(g[k], g0[k]) for k in g)
    assert np.array_equal(rec["affine"], rec0["affine"]) and torch.equal(rec["lab"], rec0["lab"]) and "zscore" not in rec0
    # one batch gathered from it, background centres by the != rule
    ld = DeviceDatasetLoader([rec], 32, 4, 1, device=dev, seed=5, pos=1.0, neg=3.0, image_rule="ne")
    batch, = list(ld)
    assert tuple(batch["image"].shape) == (4, 2, 32, 32, 32) and ld.image_rule == "ne"
    for j in range(4):
        z0, y0, x0 = (int(v) for v in ld.last_picks[j, 3:6])
        assert torch.equal(batch["image"][j], rec["img"][:, z0:z0 + 32, y0:y0 + 32, x0:x0 + 32])
        if ld.last_rows[j].mode == 0:
            flat = int(ld.last_picks[j, 7])
            zz = int(ld.last_picks[j, 6])
            assert got[0, zz].reshape(-1)[flat] != 0 and rec["lab"][zz].reshape(-1)[flat] == 0
    with pytest.raises(ValueError, match="image_rule"):
        DeviceDatasetLoader([rec], 32, 4, 1, device=dev, image_rule="ge")


@pytest.mark.parametrize("bad,clip", [(np.nan, ()), (np.inf, ("--t_zscore_clip", "0.5", "99.5"))])
def test_non_finite_intensity_is_an_error_that_names_the_file(bad, clip):
    from medicalsemseg_amd.data_device import preprocess_volume
    from medicalsemseg_amd.utils.arguments import get_args
    rng = np.random.default_rng(37)
    image = (rng.standard_normal((2, 33, 34, 35)) + 4.0).astype(np.float32)
    image[1, 5, 6, 7] = bad
    cfg = get_args(["--vol_size", "32", "--in_chans", "2", "--t_zscore", *clip])
    with pytest.raises(ValueError, match=r"case_17\.nii\.gz.*--t_zscore"):
        preprocess_volume(image, None, np.eye(4), cfg, _dev(), "case_17.nii.gz")
