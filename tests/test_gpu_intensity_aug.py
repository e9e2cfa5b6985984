"""msseg_intensity_aug on the GPU (--t_noise_prob, --t_blur_prob, --t_contrast_prob, --t_gamma_invert_prob, --t_gamma_prob):
every stage alone against the float64 restatement of tests/intensity_aug_ref.py, the generator's integer stage bit for bit,
the whole chain, the refusals, both loaders and the training driver.

Bounds.  Blur 1e-5 max|x| and contrast 1e-5 (max - min) are derived (three passes of <= 17 normalised fp32 taps; one fp32
multiply-add and a clip).  The two that cannot be derived are 4 x a measurement on these inputs (one MI355X):
  Z_ERR      max |z - float64 Box-Muller of the same uniforms| over the 4 x 5994 samples below: 3.87e-07 (at |z| = 3.4; fp32 logf, sqrtf and cospif)
  GAMMA_ERR  max |out - restatement| / (max - min) of the input over gamma in {0.7, 1.5}, plain and inverted, on both
             inputs: 1.76e-07 (powf, then the fp32 (y - mean) * scale + m)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import intensity_aug_ref as iref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 2, 9, 18, 37)            # no dimension a multiple of a tile (8 x 8 x 32 / 16), 9 barely above the largest radius
Z_ERR, GAMMA_ERR = 3.87e-07, 1.76e-07
Z_BOUND, GAMMA_BOUND = 4 * Z_ERR, 4 * GAMMA_ERR
KEYS = [0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x9E3779B97F4A7C15, 42]
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _input(kind, shape=SHAPE):
    """'unit': uniform in [0, 1]; 'zscore': normal, clipped to +-4"""
    if (kind, shape) not in _CACHE:
        rng = np.random.default_rng(71)
        x = rng.random(shape) if kind == "unit" else np.clip(rng.standard_normal(shape) * 1.3, -4.0, 4.0)
        x = x.astype(np.float32)
        x.setflags(write=False)
        _CACHE[(kind, shape)] = x
    return _CACHE[(kind, shape)]


def _row(mask=0, noise_std=0.0, noise_key=0, blur_sigma=0.0, contrast=1.0, gamma_inv=1.0, gamma=1.0):
    from medicalsemseg_amd.data_device import IntensityRow
    return IntensityRow(mask, noise_std, noise_key, blur_sigma, contrast, gamma_inv, gamma)


def _run(x, rows, dtype=torch.float32):
    from medicalsemseg_amd import hip
    out = hip.intensity_aug(torch.tensor(x, device=_dev()), rows, dtype)              # a copy: the shared inputs are read-only
    torch.cuda.synchronize()
    return out.cpu()


def _span(v):
    return float(v.max()) - float(v.min())


def _chain_bound(x, row):
    """sum of the stage bounds for one (patch, channel): the noise widens magnitude and range by at most 6 sigma a side"""
    s = float(row.noise_std) if row.mask & iref.NOISE else 0.0
    mag, span = float(np.abs(x).max()) + 6.0 * s, _span(x) + 12.0 * s
    b = s * Z_BOUND if row.mask & iref.NOISE else 0.0
    b += 1e-5 * mag if row.mask & iref.BLUR else 0.0
    b += 1e-5 * span if row.mask & iref.CONTRAST else 0.0
    b += GAMMA_BOUND * span * (bool(row.mask & iref.GAMMA_INV) + bool(row.mask & iref.GAMMA))
    return b


def _check_chain(got, x, rows, what=""):
    want = iref.apply(x, rows)
    C = x.shape[1]
    for j, row in enumerate(rows):
        n, c = divmod(j, C)
        err, bound = float(np.abs(got[n, c].astype(np.float64) - want[n, c]).max()), _chain_bound(x[n, c], row)
        print(f"{what} row {j} mask {row.mask}: max abs error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, j, err, bound)


# ---- noise --------------------------------------------------------------------------------------------------------------
def test_noise_words_are_philox4x32_10_bit_for_bit():
    from medicalsemseg_amd import hip
    for key, first in ((KEYS[0], 0), (KEYS[1], 2 ** 32 - 3), (0, 0)):
        got = hip.intensity_noise_bits(key, 5994, first, _dev()).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, iref.noise_words(key, 5994, first)), hex(key)


def _noise_fields():
    if "z" not in _CACHE:
        rows = [_row(iref.NOISE, 1.0, k) for k in KEYS]
        _CACHE["z"] = _run(np.zeros(SHAPE, dtype=np.float32), rows).numpy()
    return _CACHE["z"]


def test_noise_of_a_zero_input_is_z():
    z = _noise_fields()
    V = int(np.prod(SHAPE[2:]))
    worst = 0.0
    for j, key in enumerate(KEYS):
        want = iref.normals(key, V).reshape(SHAPE[2:])
        worst = max(worst, float(np.abs(z[j // 2, j % 2].astype(np.float64) - want).max()))
    print(f"noise: max |z - float64 Box-Muller| {worst:.3e}, bound {Z_BOUND:.3e}")
    assert worst <= Z_BOUND


def test_noise_statistics_of_the_fixed_keys():
    z = _noise_fields().astype(np.float64)
    n = int(np.prod(SHAPE[2:]))                            # N / 4 samples per (patch, channel)
    for j in range(4):
        f = z[j // 2, j % 2]
        assert abs(f.mean()) <= 5.0 / np.sqrt(n) and abs(f.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n), (j, f.mean(), f.var())
        g = (f - f.mean()) / f.std()
        for axis in range(3):
            a, b = np.moveaxis(g, axis, 0)[:-1], np.moveaxis(g, axis, 0)[1:]
            assert abs((a * b).mean()) <= 5.0 / np.sqrt(n), (j, axis, (a * b).mean())
    assert not np.array_equal(z[0, 0], z[0, 1]) and abs(np.corrcoef(z[0, 0].ravel(), z[0, 1].ravel())[0, 1]) <= 5.0 / np.sqrt(n)


def test_noise_depends_on_key_and_voxel_only():
    x = _input("zscore")
    rows = [_row(iref.NOISE, 0.5, KEYS[0]), _row(iref.NOISE, 0.5, KEYS[1]), _row(iref.NOISE, 0.5, KEYS[1]), _row(iref.NOISE, 0.5, KEYS[0])]
    got = _run(x, rows).numpy()
    z = _run(np.zeros(SHAPE, dtype=np.float32), rows).numpy()
    assert np.array_equal(z[0, 0], z[1, 1]) and np.array_equal(z[0, 1], z[1, 0]) and not np.array_equal(z[0, 0], z[0, 1])
    _check_chain(got, x, rows, "noise")
    # an 8^3 patch of its own: the field is the head of the same stream, whatever the grid
    small = _run(np.zeros((1, 1, 8, 8, 8), dtype=np.float32), [_row(iref.NOISE, 0.5, KEYS[0])]).numpy()
    assert np.array_equal(small.ravel(), z[0, 0].ravel()[:512])


# ---- blur ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 0.62, 1.0, 2.0])
@pytest.mark.parametrize("kind", ["unit", "zscore"])
def test_blur_is_gaussian_filter(kind, sigma):
    import scipy.ndimage as ndi
    for shape in (SHAPE, (1, 1, 8, 8, 8)):
        x = _input(kind, shape)
        got = _run(x, [_row(iref.BLUR, blur_sigma=sigma)] * (shape[0] * shape[1])).numpy()
        bound = 1e-5 * float(np.abs(x).max())
        for n in range(shape[0]):
            for c in range(shape[1]):
                want = ndi.gaussian_filter(x[n, c].astype(np.float64), float(np.float32(sigma)), mode="reflect", truncate=4.0)
                err = float(np.abs(got[n, c] - want).max())
                print(f"blur {kind} sigma {sigma} {shape[2:]}: max abs error {err:.3e}, bound {bound:.3e}")
                assert err <= bound


def test_blur_radii_may_differ_between_rows():
    x = _input("zscore")
    rows = [_row(iref.BLUR, blur_sigma=2.0), _row(0), _row(iref.BLUR, blur_sigma=0.5), _row(iref.BLUR, blur_sigma=1.0)]
    got = _run(x, rows).numpy()
    _check_chain(got, x, rows, "mixed radii")
    assert np.array_equal(got[0, 1], x[0, 1])


@pytest.mark.parametrize("sigma", [0.62, 2.0])
def test_noise_and_blur_together_blur_the_noisy_volume(sigma):
    """a halo voxel carries the noise of the voxel it mirrors: the result is the blur of (input + noise field)"""
    import scipy.ndimage as ndi
    x = _input("zscore")
    rows = [_row(iref.NOISE | iref.BLUR, 0.1, k, sigma) for k in KEYS]
    got = _run(x, rows).numpy()
    for j, row in enumerate(rows):
        noisy = x[j // 2, j % 2].astype(np.float64) + float(np.float32(0.1)) * iref.normals(row.noise_key, x[0, 0].size).reshape(x.shape[2:])
        want = ndi.gaussian_filter(noisy, float(np.float32(sigma)), mode="reflect", truncate=4.0)
        err, bound = float(np.abs(got[j // 2, j % 2] - want).max()), 1e-5 * float(np.abs(noisy).max()) + 0.1 * Z_BOUND
        print(f"noise + blur sigma {sigma} row {j}: max abs error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


# ---- contrast, gamma ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0.75, 1.25])
@pytest.mark.parametrize("kind", ["unit", "zscore"])
def test_contrast(kind, f):
    x = _input(kind)
    got = _run(x, [_row(iref.CONTRAST, contrast=f)] * 4).numpy()
    for n in range(2):
        for c in range(2):
            err, bound = float(np.abs(got[n, c] - iref.contrast(x[n, c], f)).max()), 1e-5 * _span(x[n, c])
            print(f"contrast {kind} {f}: max abs error {err:.3e}, bound {bound:.3e}")
            assert err <= bound and got[n, c].min() >= x[n, c].min() and got[n, c].max() <= x[n, c].max()
    assert float(np.abs(got - x).max()) > 1e-3


@pytest.mark.parametrize("g", [0.7, 1.5])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("kind", ["unit", "zscore"])
def test_gamma(kind, invert, g):
    x = _input(kind)
    row = _row(iref.GAMMA_INV, gamma_inv=g) if invert else _row(iref.GAMMA, gamma=g)
    got = _run(x, [row] * 4).numpy().astype(np.float64)
    for n in range(2):
        for c in range(2):
            span = _span(x[n, c])
            err = float(np.abs(got[n, c] - iref.gamma(x[n, c], float(np.float32(g)), invert)).max())
            xm, xs = x[n, c].astype(np.float64).mean(), x[n, c].astype(np.float64).std()
            print(f"gamma {kind} invert {invert} {g}: max abs error / span {err / span:.3e}, bound {GAMMA_BOUND:.3e}; "
                  f"mean off by {abs(got[n, c].mean() - xm):.3e}, std off by {abs(got[n, c].std() - xs):.3e}")
            assert err <= GAMMA_BOUND * span
            assert abs(got[n, c].mean() - xm) <= GAMMA_BOUND * span and abs(got[n, c].std() - xs) <= GAMMA_BOUND * span
    assert float(np.abs(got - x).max()) > 1e-3


def test_a_constant_channel_comes_back_bit_identical():
    x = _input("zscore").copy()
    x[0, 1] = np.float32(0.37)
    x[1, 0] = np.float32(-2.5)
    rows = [_row(iref.GAMMA | iref.GAMMA_INV | iref.CONTRAST, contrast=1.25, gamma_inv=0.7, gamma=1.5)] * 4
    for dtype in (torch.float32, torch.bfloat16):
        got = _run(x, rows, dtype)
        want = torch.from_numpy(x).to(dtype)
        assert torch.equal(got[0, 1], want[0, 1]) and torch.equal(got[1, 0], want[1, 0]) and not torch.equal(got[0, 0], want[0, 0])
        assert bool(torch.isfinite(got.float()).all())


# ---- the whole chain --------------------------------------------------------------------------------------------------------
def _chain_rows():
    return [_row(31, 0.1, KEYS[0], 1.0, 1.25, 1.5, 0.7), _row(31, 0.05, KEYS[1], 0.62, 0.75, 0.7, 1.5),
            _row(0), _row(31, 0.1, KEYS[3], 2.0, 1.1, 1.2, 0.8)]


@pytest.mark.parametrize("kind", ["unit", "zscore"])
def test_full_chain(kind):
    x, rows = _input(kind), _chain_rows()
    got = _run(x, rows)
    _check_chain(got.numpy(), x, rows, "chain " + kind)
    assert torch.equal(got, _run(x, rows))                                           # two calls, the same bits
    assert torch.equal(_run(x, rows, torch.bfloat16), got.to(torch.bfloat16))
    assert np.array_equal(got[1, 0].numpy(), x[1, 0]) and not np.array_equal(got[0, 1].numpy(), x[0, 1])   # row 2 has no bit set
    one = (1, 1, 8, 8, 8)
    _check_chain(_run(_input(kind, one), rows[:1]).numpy(), _input(kind, one), rows[:1], "chain 8^3 " + kind)


@pytest.mark.parametrize("mask", [iref.NOISE | iref.CONTRAST, iref.BLUR | iref.GAMMA, iref.CONTRAST | iref.GAMMA_INV,
                                  iref.NOISE | iref.GAMMA_INV | iref.GAMMA])
def test_partial_chains_read_the_right_statistics(mask):
    """the statistics a stage reads are those of the last stage that wrote the row, whichever stages the row skips"""
    x = _input("zscore")
    rows = [_row(mask, 0.1, KEYS[2], 1.0, 1.25, 1.5, 0.7), _row(31, 0.1, KEYS[0], 0.5, 0.75, 0.7, 1.5), _row(0),
            _row(mask & ~iref.GAMMA, 0.1, KEYS[1], 0.62, 0.75, 0.7, 1.5)]
    for dtype in (torch.float32, torch.bfloat16):
        got = _run(x, rows, dtype)
        if dtype == torch.float32:
            _check_chain(got.numpy(), x, rows, f"mask {mask}")
            ref = got
        else:
            assert torch.equal(got, ref.to(torch.bfloat16))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from medicalsemseg_amd import hip
    dev = _dev()
    blur = _row(iref.BLUR, blur_sigma=1.0)

    def refused(exc, x, rows, match):
        out = torch.full(x.shape, 7.0, device=dev)
        with pytest.raises(exc, match=match):
            hip.intensity_aug(x, rows, torch.float32, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    ok = torch.zeros(1, 1, 8, 8, 8, device=dev)
    refused(hip.MssegError, torch.zeros(1, 1, 7, 8, 8, device=dev), [blur], "dimension")
    refused(hip.MssegError, torch.zeros(1, 1, 8, 8, 7, device=dev), [_row(0)], "dimension")
    refused(hip.MssegError, ok, [_row(iref.BLUR, blur_sigma=2.1)], "sigma")
    refused(hip.MssegError, ok, [_row(iref.GAMMA, gamma=0.0)], "gamma")
    refused(RuntimeError, torch.zeros(1, 1, 8, 8, 8), [blur], "GPU")
    refused(TypeError, ok.half(), [blur], "float32")
    refused(ValueError, torch.zeros(1, 8, 8, 8, 2, device=dev).permute(0, 4, 1, 2, 3), [blur, blur], "contiguous")
    refused(ValueError, ok, [blur, blur], "rows")
    with pytest.raises(TypeError):
        hip.intensity_aug(ok, [blur], torch.float16)
    hip.intensity_aug(ok, [_row(iref.BLUR, blur_sigma=2.0)], torch.float32)           # the limit itself runs
    torch.cuda.synchronize()


# ---- loaders ----------------------------------------------------------------------------------------------------------------
ALL_ON = dict(noise_prob=1.0, blur_prob=1.0, blur_channel_prob=1.0, contrast_prob=1.0, gamma_invert_prob=1.0, gamma_prob=1.0)
VOL_SHAPES = [(33, 41, 36), (37, 30, 31), (31, 35, 40)]


def _records(dev):
    if "recs" not in _CACHE:
        rng = np.random.default_rng(72)
        recs = []
        for k, shape in enumerate(VOL_SHAPES):
            img = torch.from_numpy(rng.standard_normal((2,) + shape).astype(np.float32)).to(dev)
            lab = torch.from_numpy(rng.integers(0, 3, shape).astype(np.uint8)).to(dev)
            recs.append({"img": img, "lab": lab, "affine": np.eye(4), "original_affine": np.eye(4), "filename": f"/data/v{k}.nii.gz"})
        _CACHE["recs"] = recs
    return _CACHE["recs"]


@pytest.mark.parametrize("affine", [0.0, 1.0])
def test_device_dataset_loader_with_intensity(affine):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import DeviceDatasetLoader, _upload, intensity_config
    dev = _dev()
    recs = _records(dev)
    roi, batch = 16, 2
    kw = dict(patches_per_image=1, device=dev, seed=31, flip_prob=0.5, rot_prob=0.5, shift_prob=0.5, scale_prob=0.5,
              affine_prob=affine, affine_pad=-0.5)
    ld = DeviceDatasetLoader(recs, roi, batch, 2, intensity=intensity_config(**ALL_ON), **kw)
    images = []
    for b in ld:
        assert len(ld.last_intensity) == batch * 2 and all(r.mask == 31 for r in ld.last_intensity)
        img = torch.empty(batch, 2, roi, roi, roi, device=dev)
        lab = torch.empty(batch, 1, roi, roi, roi, device=dev)
        table, picks = _upload(ld.last_rows, dev), ld.last_picks.to(dev)
        if affine:
            hip.aug_crop_affine(ld.desc, len(recs), table, picks, torch.from_numpy(ld.last_mats).to(dev), img, lab, roi, -0.5)
        else:
            assert ld.last_mats is None
            hip.aug_crop_multi(ld.desc, len(recs), table, picks, img, lab, roi)
        assert torch.equal(b["label"], lab) and b["image"].dtype == torch.float32
        _check_chain(b["image"].cpu().numpy(), img.cpu().numpy(), ld.last_intensity, f"dataset loader affine {affine}")
        assert not torch.equal(b["image"], img)
        images.append(b["image"].clone())
    again = [b["image"].clone() for b in DeviceDatasetLoader(recs, roi, batch, 2, intensity=intensity_config(**ALL_ON), **kw)]
    assert all(torch.equal(p, q) for p, q in zip(images, again))
    # every stage off: the parent's batches and generator stream, no rows kept; bf16 goes through the same path
    off = DeviceDatasetLoader(recs, roi, batch, 2, intensity=intensity_config(), **kw)
    plain = DeviceDatasetLoader(recs, roi, batch, 2, **kw)
    assert all(torch.equal(p["image"], q["image"]) and torch.equal(p["label"], q["label"]) for p, q in zip(off, plain))
    assert off.last_intensity is None and off.rng.bit_generator.state == plain.rng.bit_generator.state
    half = DeviceDatasetLoader(recs, roi, batch, 2, out_dtype=torch.bfloat16, intensity=intensity_config(**ALL_ON), **kw)
    assert all(torch.equal(b["image"], p.to(torch.bfloat16)) for b, p in zip(half, images))


@pytest.mark.parametrize("affine", [0.0, 1.0])
def test_device_patch_loader_with_intensity(affine):
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import DevicePatchLoader, PICK_VOXEL, PickRow, _upload, intensity_config
    dev = _dev()
    rec = _records(dev)[0]
    roi, batch = 16, 2
    kw = dict(seed=32, flip_prob=0.5, rot_prob=0.5, shift_prob=0.5, scale_prob=0.5, affine_prob=affine, affine_pad=0.25)
    ld = DevicePatchLoader(rec["img"], rec["lab"], roi, batch, 2, dev, intensity=intensity_config(**ALL_ON), **kw)
    for b in ld:
        img = torch.empty(batch, 2, roi, roi, roi, device=dev)
        lab = torch.empty(batch, 1, roi, roi, roi, device=dev)
        if affine:
            table = _upload([PickRow(0, PICK_VOXEL, 0, 0, r.flips, r.rotk, r.shift, r.scale) for r in ld.last_rows], dev)
            hip.aug_crop_affine(ld.desc, 1, table, ld.last_picks.to(dev), torch.from_numpy(ld.last_mats).to(dev), img, lab, roi, 0.25)
        else:
            hip.aug_crop_batch(ld.img, ld.lab, _upload(ld.last_rows, dev), img, lab, roi)
        assert torch.equal(b["label"], lab) and len(ld.last_intensity) == batch * 2
        _check_chain(b["image"].cpu().numpy(), img.cpu().numpy(), ld.last_intensity, f"patch loader affine {affine}")
        assert not torch.equal(b["image"], img)
    off = DevicePatchLoader(rec["img"], rec["lab"], roi, batch, 2, dev, intensity=intensity_config(), **kw)
    plain = DevicePatchLoader(rec["img"], rec["lab"], roi, batch, 2, dev, **kw)
    assert all(torch.equal(p["image"], q["image"]) and torch.equal(p["label"], q["label"]) for p, q in zip(off, plain))
    assert off.last_intensity is None and off.rng.bit_generator.state == plain.rng.bit_generator.state


# ---- the training driver ------------------------------------------------------------------------------------------------------
def test_run_training_synthetic_with_intensity(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "run_training.py"), "--synthetic", "--model", "UNetSmall", "--output_dim", "2",
           "--vol_size", "32", "--n_images_per_batch", "2", "--synthetic_steps", "2", "--epochs", "2", "--val_interval", "2",
           "--synthetic_val_size", "48", "--warmup_epochs", "0", "--output_dir", str(tmp_path), "--t_rand_crop_fgbg",
           "--t_noise_prob", "1", "--t_blur_prob", "1", "--t_contrast_prob", "1", "--t_gamma_invert_prob", "1", "--t_gamma_prob", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    log = [json.loads(l) for l in open(os.path.join(str(tmp_path), "log.txt"))]
    assert len(log) == 2 and all(np.isfinite(e["train/loss"]) for e in log), log
