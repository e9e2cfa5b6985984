"""Host side of --t_zscore / --t_zscore_clip: flag parsing, every error of zscore_config, the refusals that stay, and the
numpy restatement (tests/zscore_ref.py) against numpy's own percentile / mean / std on float64 copies."""
import numpy as np
import pytest

from tests import zscore_ref as zr


def _args(*argv):
    from medicalsemseg_amd.utils.arguments import get_args
    return get_args(list(argv))


def test_flags_parse_and_default_off():
    from medicalsemseg_amd.data_device import zscore_config
    cfg = _args()
    assert cfg.t_zscore is False and cfg.t_zscore_clip == () and zscore_config(cfg) is None
    assert zscore_config(_args("--t_zscore")) == ()
    cfg = _args("--t_zscore", "--t_zscore_clip", "0.5", "99.5")
    assert cfg.t_zscore is True and cfg.t_zscore_clip == (0.5, 99.5) and zscore_config(cfg) == (0.5, 99.5)
    assert zscore_config(_args("--t_zscore", "--t_zscore_clip", "0", "100")) == (0.0, 100.0)


def test_zscore_excludes_t_normalize_and_names_both():
    from medicalsemseg_amd.data_device import check_transform_flags, zscore_config
    with pytest.raises(ValueError, match=r"--t_zscore.*--t_normalize"):
        zscore_config(_args("--t_zscore", "--t_normalize"))
    with pytest.raises(ValueError, match=r"--t_zscore.*--t_normalize"):
        check_transform_flags(_args("--t_zscore", "--t_normalize"))           # what every driver goes through


@pytest.mark.parametrize("argv", [("--t_zscore_clip", "0.5", "99.5"),                        # without --t_zscore
                                  ("--t_zscore", "--t_zscore_clip", "0.5"),                  # wrong count
                                  ("--t_zscore", "--t_zscore_clip", "0.5", "50", "99.5"),
                                  ("--t_zscore", "--t_zscore_clip", "99.5", "0.5"),          # out of order
                                  ("--t_zscore", "--t_zscore_clip", "5", "5"),
                                  ("--t_zscore", "--t_zscore_clip", "-1", "99"),             # out of range
                                  ("--t_zscore", "--t_zscore_clip", "1", "100.5"),
                                  ("--t_zscore", "--t_zscore_clip", "nan", "99")])
def test_clip_errors_name_the_flag(argv):
    from medicalsemseg_amd.data_device import zscore_config
    with pytest.raises(ValueError, match="--t_zscore_clip"):
        zscore_config(_args(*argv))


def test_reference_flags_stay_refused_and_name_themselves():
    from medicalsemseg_amd.data_device import check_transform_flags
    with pytest.raises(NotImplementedError, match="t_percentile_ct_intensity"):
        check_transform_flags(_args("--t_percentile_ct_intensity"))
    with pytest.raises(NotImplementedError, match="t_normalize_channel_wise"):
        check_transform_flags(_args("--t_normalize", "--t_normalize_channel_wise"))
    with pytest.raises(NotImplementedError, match="t_percentile_ct_intensity"):
        check_transform_flags(_args("--t_percentile_ct_intensity", "--t_zscore"))
    check_transform_flags(_args("--t_zscore", "--t_zscore_clip", "0.5", "99.5"))


def test_normalised_zero_is_zero_under_zscore():
    from medicalsemseg_amd.data_device import normalised_zero
    assert normalised_zero(_args("--t_zscore")) == 0.0


def test_loader_rule_names():
    from medicalsemseg_amd import hip
    assert hip.BG_RULES == {"gt": 0, "ne": 1}
    with pytest.raises(ValueError, match="'gt'.*'ne'"):
        hip._bg_rule("ge")


def _ulp_apart(a, b):
    """distance of two finite float32 values in units in the last place"""
    def key(v):
        i = int(np.float32(v).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))


@pytest.mark.parametrize("n", [1, 2, 3, 200, 201, 4097])
@pytest.mark.parametrize("scale", [1.0, 3000.0])
def test_percentile_within_one_ulp_of_numpy(n, scale):
    rng = np.random.default_rng(n)
    s = np.sort((rng.standard_normal(n) * scale).astype(np.float32))
    for q in (0.0, 0.5, 2.0, 50.0, 97.3, 99.5, 100.0):
        want = np.percentile(s.astype(np.float64), q)
        got = zr.percentile_f32(s, q)
        assert got.dtype == np.float32 and _ulp_apart(got, np.float32(want)) <= 1, (n, q, got, want)


def test_percentile_100_clamps_the_upper_rank_and_n_1():
    s = np.array([-3.0, 1.0, 2.5, 7.0], dtype=np.float32)
    assert zr.ranks_of(100.0, 4) == (3, 3, 0.0) and zr.percentile_f32(s, 100.0) == np.float32(7.0)
    assert zr.ranks_of(0.0, 4) == (0, 1, 0.0) and zr.percentile_f32(s, 0.0) == np.float32(-3.0)
    one = np.array([4.25], dtype=np.float32)
    for q in (0.0, 0.5, 50.0, 100.0):
        assert zr.ranks_of(q, 1) == (0, 0, 0.0) and zr.percentile_f32(one, q) == np.float32(4.25)
    one_voxel = np.array([0.0, 4.25, 0.0], dtype=np.float32)
    assert zr.channel_stats(one_voxel, (0.5, 99.5)) == (1, 4.25, 4.25, 4.25, 1.0)            # std 0 -> 1


@pytest.mark.parametrize("clip", [None, (0.5, 99.5), (10.0, 60.0)])
def test_stats_and_apply_against_numpy_float64(clip):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((9, 11, 13)) * 40.0 + 300.0).astype(np.float32)
    x[rng.random(x.shape) < 0.3] = 0.0
    x[0, 0, :4] = -0.0
    n, lo, hi, mean, std = zr.channel_stats(x, clip)
    v = x[x != 0].astype(np.float64)
    assert n == v.size == int(np.count_nonzero(x))
    if clip is not None:
        p = np.percentile(v, clip)
        assert _ulp_apart(lo, np.float32(p[0])) <= 1 and _ulp_apart(hi, np.float32(p[1])) <= 1
        v = np.clip(v, float(lo), float(hi))
    else:
        assert lo == -np.inf and hi == np.inf
    assert abs(mean - np.mean(v)) <= 1e-12 * abs(np.mean(v)) and abs(std - np.std(v)) <= 1e-12 * np.std(v)
    out, stats = zr.zscore_nonzero(x[None], clip)
    assert out.dtype == np.float32 and np.array_equal(stats[0], [n, lo, hi, mean, std])
    assert np.array_equal(out[0][x == 0].view(np.uint32), x[x == 0].view(np.uint32))      # -0.0 and 0.0 keep their bits
    want = (v - np.mean(v)) / np.std(v)
    assert np.abs(out[0][x != 0] - want).max() <= 1e-5
    assert abs(out[0][x != 0].astype(np.float64).mean()) < 1e-5


def test_empty_and_constant_channels():
    z = np.zeros((3, 4, 5), dtype=np.float32)
    out, stats = zr.zscore_nonzero(z[None], (0.5, 99.5))
    assert np.array_equal(out[0], z) and stats[0].tolist() == [0.0, -np.inf, np.inf, 0.0, 1.0]
    c = np.where(np.arange(60).reshape(3, 4, 5) % 2 == 0, np.float32(7.5), np.float32(0.0)).astype(np.float32)
    out, stats = zr.zscore_nonzero(c[None])
    assert stats[0].tolist() == [30.0, -np.inf, np.inf, 7.5, 1.0] and np.array_equal(out[0], np.zeros_like(c))
