"""Host side of the affine crop gather (--t_affine_prob): the numpy restatement of tests/affine_ref.py against
scipy.ndimage.affine_transform in float64, the matrix builder, the flags and their validation, and the generator stream of
the draws.  No GPU."""
import numpy as np
import pytest

from tests import affine_ref as aref

# volume shape, roi, crop start, seed
CASES = [((20, 33, 41), 16, (0, 0, 0), 101), ((20, 33, 41), 16, (4, 17, 25), 102),
         ((37, 30, 31), 30, (7, 0, 1), 103), ((19, 23, 29), 15, (2, 4, 7), 104)]
PAD = -0.6974


def _case(shape, seed):
    rng = np.random.default_rng(seed)
    img = rng.uniform(-1.0, 1.0, (2,) + shape).astype(np.float32)
    lab = rng.integers(0, 5, shape).astype(np.uint8)
    return rng, img, lab


@pytest.mark.parametrize("shape,roi,start,seed", CASES)
def test_restatement_matches_scipy_affine_transform(shape, roi, start, seed):
    """image within 64 * 2^-24 * max(|v|, |pad|) of scipy in float64 with order=1, mode="grid-constant": seven fp32 lerps of
    two or three roundings each plus the fraction's cast to float; labels equal to order=0 wherever no coordinate lies within
    1e-6 of a half-integer, and for these seeds no voxel is excluded that way"""
    from scipy import ndimage
    rng, img, lab = _case(shape, seed)
    assert float(np.abs(img).max()) <= 1.0
    from medicalsemseg_amd.data_device import affine_matrix
    # three random matrices and a near-extreme one (large angles, the widest field of view), which reaches outside every
    # volume (not 30 degrees: sin 30 = 0.5 puts coordinates on exact half-integers)
    for m in [aref.random_matrix(rng) for _ in range(3)] + [affine_matrix(np.deg2rad([29.0, -28.0, 27.0]), 0.7)]:
        got_i, got_l = aref.affine_crop(img, lab, start, roi, 0, 0, 0.0, 1.0, m, PAD)
        h = (roi - 1) / 2.0
        offset = (np.asarray(start, dtype=np.float64) + h) - m @ np.full(3, h)
        want_i = np.stack([ndimage.affine_transform(img[c].astype(np.float64), m, offset=offset, output_shape=(roi,) * 3, order=1,
                                                    mode="grid-constant", cval=PAD) for c in range(img.shape[0])])
        want_l = ndimage.affine_transform(lab, m, offset=offset, output_shape=(roi,) * 3, order=0, mode="grid-constant", cval=0)
        bound = 64 * 2.0 ** -24 * max(float(np.abs(img).max()), abs(PAD))
        err = float(np.abs(got_i.astype(np.float64) - want_i).max())
        print(f"{shape} roi {roi} start {start}: image error {err:.3e} (bound {bound:.3e})")
        assert got_i.dtype == np.float32 and err <= bound
        coords = aref.source_coords(start, roi, 0, 0, m)
        assert aref.half_integer_share(coords) == 0.0
        assert np.array_equal(got_l, want_l.astype(np.float32))
    assert coords.min() < -1.0                                   # the last matrix: whole taps outside the volume


def test_restatement_with_identity_is_the_plain_crop():
    from oracle.augment import apply_row
    rng, img, lab = _case((20, 33, 41), 105)
    for flips, rotk, start in [(0, 0, (4, 17, 25)), (5, 1, (0, 0, 0)), (2, 3, (4, 17, 25)), (7, 2, (9, 40, 60))]:
        got_i, got_l = aref.affine_crop(img, lab, start, 16, flips, rotk, 0.05, 1.1, np.eye(3), PAD)
        s = aref.clamp_start(start, 16, lab.shape)
        want_i, want_l = apply_row(img, lab, s, 16, (flips & 1, flips & 2, flips & 4), rotk, 0.05, 1.1)
        assert np.array_equal(got_i.view(np.uint32), want_i.view(np.uint32)) and np.array_equal(got_l, want_l)


def test_affine_matrix_is_a_scaled_rotation():
    from medicalsemseg_amd.data_device import affine_matrix
    rng = np.random.default_rng(106)
    for _ in range(50):
        ang, zoom = rng.uniform(-np.pi, np.pi, 3), float(rng.uniform(0.5, 2.0))
        m = affine_matrix(ang, zoom)
        assert m.dtype == np.float64 and m.shape == (3, 3)
        assert np.abs(m @ m.T - np.eye(3) / zoom ** 2).max() <= 1e-12
        assert abs(np.linalg.det(m) - zoom ** -3) <= 1e-12
    m = affine_matrix((0.0, 0.0, 0.0), 1.0)
    assert np.array_equal(m, np.eye(3)) and not np.signbit(m).any()
    # right-handed about tensor axis 0 of (D, H, W): a quarter turn takes the H axis onto the W axis
    q = affine_matrix((np.pi / 2, 0.0, 0.0), 1.0)
    assert np.allclose(q @ np.array([0.0, 1.0, 0.0]), [0.0, 0.0, 1.0], atol=1e-15)
    assert np.allclose(affine_matrix((0.0, np.pi / 2, 0.0), 1.0) @ np.array([0.0, 0.0, 1.0]), [1.0, 0.0, 0.0], atol=1e-15)
    assert np.allclose(affine_matrix((0.0, 0.0, np.pi / 2), 2.0) @ np.array([1.0, 0.0, 0.0]), [0.0, 0.5, 0.0], atol=1e-15)


def test_flags_defaults_and_validation():
    from medicalsemseg_amd.data_device import affine_config
    from medicalsemseg_amd.utils.arguments import get_args
    cfg = get_args([])
    assert cfg.t_affine_prob == 0.0 and cfg.t_affine_rotate == 30.0 and cfg.t_affine_zoom == (0.7, 1.4)
    assert affine_config(cfg.t_affine_prob, cfg.t_affine_rotate, cfg.t_affine_zoom) == (0.0, (30.0, 30.0, 30.0), (0.7, 1.4))
    cfg = get_args("--t_affine_prob 0.25 --t_affine_rotate 10 0 25.5 --t_affine_zoom 0.9 1.1".split())
    assert affine_config(cfg.t_affine_prob, cfg.t_affine_rotate, cfg.t_affine_zoom) == (0.25, (10.0, 0.0, 25.5), (0.9, 1.1))
    assert affine_config(1, 15, [1.0, 1.0]) == (1.0, (15.0, 15.0, 15.0), (1.0, 1.0))
    for prob in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="t_affine_prob"):
            affine_config(prob, 30.0, (0.7, 1.4))
    for rot in (-1.0, (10.0, 20.0), (10.0, -1.0, 5.0), (), (1.0, 2.0, 3.0, 4.0), float("nan")):
        with pytest.raises(ValueError, match="t_affine_rotate"):
            affine_config(0.5, rot, (0.7, 1.4))
    for zoom in (1.0, (0.0, 1.0), (1.4, 0.7), (-1.0, 1.0), (0.7, 1.0, 1.4), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="t_affine_zoom"):
            affine_config(0.5, 30.0, zoom)


def test_loaders_validate_the_affine_arguments_before_anything_else():
    """the ValueError comes at construction, before the loader touches a device"""
    from medicalsemseg_amd.data_device import DeviceDatasetLoader
    with pytest.raises(ValueError, match="t_affine_prob"):
        DeviceDatasetLoader([], 16, 1, 1, affine_prob=2.0)
    with pytest.raises(ValueError, match="t_affine_zoom"):
        DeviceDatasetLoader([], 16, 1, 1, affine_prob=0.5, affine_zoom=(1.4, 0.7))


CFG = dict(pos=2.0, neg=1.0, flip_prob=0.5, rot_prob=0.6, shift_os=0.1, shift_prob=0.5, scale_f=0.1, scale_prob=0.5)


def test_probability_zero_leaves_the_generator_stream_alone():
    from medicalsemseg_amd.data_device import affine_config, draw_affine, draw_rows
    a, b = np.random.default_rng(31), np.random.default_rng(31)
    rows_a = draw_rows(a, 6, 100, 200, CFG)
    rows_b = draw_rows(b, 6, 100, 200, CFG)
    mats = draw_affine(b, 6, affine_config(0.0, 30.0, (0.7, 1.4)))
    assert rows_a == rows_b and np.array_equal(mats, np.tile(np.eye(3), (6, 1, 1)))
    assert a.bit_generator.state == b.bit_generator.state
    assert a.random() == b.random()


def test_draw_order_one_uniform_then_three_angles_and_the_zoom_only_if_chosen():
    from medicalsemseg_amd.data_device import affine_config, affine_matrix, draw_affine
    aff = affine_config(0.5, (30.0, 10.0, 20.0), (0.7, 1.4))
    got = draw_affine(np.random.default_rng(32), 40, aff)
    rng, chosen = np.random.default_rng(32), 0
    for j in range(40):
        want = np.eye(3)
        if rng.random() < 0.5:
            ang = [np.deg2rad(rng.uniform(-a, a)) for a in (30.0, 10.0, 20.0)]
            want = affine_matrix(ang, rng.uniform(0.7, 1.4))
            chosen += 1
        assert np.array_equal(got[j], want), j
    assert 8 <= chosen <= 32
    every = draw_affine(np.random.default_rng(33), 20, affine_config(1.0, 30.0, (0.7, 1.4)))
    assert all(not np.array_equal(m, np.eye(3)) for m in every)
    zooms = np.cbrt(1.0 / np.linalg.det(every))
    assert zooms.min() >= 0.7 - 1e-12 and zooms.max() <= 1.4 + 1e-12
