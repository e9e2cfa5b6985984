"""Host side of the intensity augmentation (--t_noise_prob, --t_blur_prob, --t_contrast_prob, --t_gamma_invert_prob,
--t_gamma_prob): the flags, their validation, the draws of draw_intensity, the float64 restatement of
tests/intensity_aug_ref.py against scipy and against its own invariants, and the row layout of include/msseg.h."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

from medicalsemseg_amd.data_device import (IntensityRow, draw_intensity, intensity_config, intensity_config_from_args,
                                           intensity_on)
from medicalsemseg_amd.utils.arguments import get_args
from tests import intensity_aug_ref as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ON = dict(noise_prob=1.0, blur_prob=1.0, blur_channel_prob=1.0, contrast_prob=1.0, gamma_invert_prob=1.0, gamma_prob=1.0)


def test_flags_parse_with_the_documented_defaults():
    cfg = get_args([])
    assert (cfg.t_noise_prob, cfg.t_blur_prob, cfg.t_contrast_prob, cfg.t_gamma_invert_prob, cfg.t_gamma_prob) == (0.0,) * 5
    assert cfg.t_noise_std == (0.0, 0.1) and cfg.t_blur_sigma == (0.5, 1.0) and cfg.t_blur_channel_prob == 0.5
    assert cfg.t_contrast_range == (0.75, 1.25) and cfg.t_gamma_range == (0.7, 1.5)
    conf = intensity_config_from_args(cfg)
    assert conf == intensity_config() and not intensity_on(conf)
    cfg = get_args("--t_noise_prob 0.1 --t_noise_std 0 0.05 --t_blur_prob 0.2 --t_blur_sigma 0.5 1.5 --t_blur_channel_prob 1 "
                   "--t_contrast_prob 0.15 --t_contrast_range 0.65 1.5 --t_gamma_invert_prob 0.1 --t_gamma_prob 0.3 "
                   "--t_gamma_range 0.7 1.5".split())
    conf = intensity_config_from_args(cfg)
    assert intensity_on(conf) and conf["noise_std"] == (0.0, 0.05) and conf["blur_sigma"] == (0.5, 1.5)
    assert conf["blur_channel_prob"] == 1.0 and conf["contrast_range"] == (0.65, 1.5) and conf["gamma_prob"] == 0.3


@pytest.mark.parametrize("flag", ["noise_prob", "blur_prob", "blur_channel_prob", "contrast_prob", "gamma_invert_prob",
                                  "gamma_prob"])
def test_a_probability_outside_0_1_names_its_flag(flag):
    for bad in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="t_" + flag):
            intensity_config(**{flag: bad})


@pytest.mark.parametrize("flag, bad", [("noise_std", (0.2, 0.1)), ("noise_std", (-0.1, 0.1)), ("blur_sigma", (1.0, 0.5)),
                                       ("blur_sigma", (0.5, 2.1)), ("blur_sigma", (0.0, 1.0)), ("contrast_range", (1.25, 0.75)),
                                       ("gamma_range", (1.5, 0.7)), ("gamma_range", (0.0, 1.5)), ("gamma_range", (0.7,)),
                                       ("contrast_range", 1.0)])
def test_a_bad_range_names_its_flag(flag, bad):
    with pytest.raises(ValueError, match="t_" + flag):
        intensity_config(**{flag: bad})
    assert intensity_config(blur_sigma=(0.5, 2.0))["blur_sigma"] == (0.5, 2.0)       # the kernel's limit itself is allowed


def test_every_probability_zero_leaves_the_generator_alone():
    rng = np.random.default_rng(5)
    before = rng.bit_generator.state
    rows = draw_intensity(rng, 3, 2, intensity_config())
    assert rng.bit_generator.state == before
    assert len(rows) == 6 and all(r.mask == 0 for r in rows)
    # a stage of probability 0 draws nothing: contrast alone consumes what contrast alone needs (1 + 2 per channel)
    a, b = np.random.default_rng(6), np.random.default_rng(6)
    draw_intensity(a, 1, 2, intensity_config(contrast_prob=1.0))
    b.random(5)
    assert a.bit_generator.state == b.bit_generator.state


def test_draws_lie_in_their_ranges_and_repeat_with_the_seed():
    conf = intensity_config(noise_std=(0.02, 0.1), blur_sigma=(0.5, 1.0), contrast_range=(0.75, 1.25), gamma_range=(0.7, 1.5), **ALL_ON)
    rows = draw_intensity(np.random.default_rng(7), 200, 3, conf)
    again = draw_intensity(np.random.default_rng(7), 200, 3, conf)
    assert len(rows) == 600 and [bytes(r) for r in rows] == [bytes(r) for r in again]
    assert bytes(draw_intensity(np.random.default_rng(8), 200, 3, conf)[0]) != bytes(rows[0])
    assert all(r.mask == 31 for r in rows)
    f32 = np.float32
    assert all(f32(0.02) <= r.noise_std <= f32(0.1) for r in rows) and all(f32(0.5) <= r.blur_sigma <= f32(1.0) for r in rows)
    assert all(f32(0.75) <= r.contrast <= f32(1.25) for r in rows)
    assert all(f32(0.7) <= r.gamma <= f32(1.5) and f32(0.7) <= r.gamma_inv <= f32(1.5) for r in rows)
    # one std per patch, one key per channel; both sides of 1 occur
    for j in range(200):
        p = rows[3 * j:3 * j + 3]
        assert p[0].noise_std == p[1].noise_std == p[2].noise_std and len({r.noise_key for r in p}) == 3
    assert len({r.noise_key for r in rows}) == 600
    for field in ("contrast", "gamma", "gamma_inv"):
        v = np.array([getattr(r, field) for r in rows])
        assert (v < 1).any() and (v > 1).any()


def test_the_two_sided_rule_never_leaves_a_range_above_one():
    conf = intensity_config(contrast_range=(1.0, 1.5), gamma_range=(1.2, 1.5), **ALL_ON)
    rows = draw_intensity(np.random.default_rng(9), 300, 1, conf)
    assert all(np.float32(1.0) <= r.contrast <= np.float32(1.5) for r in rows)
    assert all(np.float32(1.2) <= r.gamma <= np.float32(1.5) and np.float32(1.2) <= r.gamma_inv <= np.float32(1.5) for r in rows)
    # and a range below one stays below
    rows = draw_intensity(np.random.default_rng(9), 300, 1, intensity_config(contrast_range=(0.5, 0.9), **ALL_ON))
    assert all(np.float32(0.5) <= r.contrast <= np.float32(0.9) for r in rows)


def test_the_channel_probability_selects_channels_of_a_chosen_patch():
    rows = draw_intensity(np.random.default_rng(10), 400, 2, intensity_config(blur_prob=1.0, blur_channel_prob=0.5))
    share = np.mean([bool(r.mask & iref.BLUR) for r in rows])
    assert abs(share - 0.5) <= 5 * 0.5 / np.sqrt(800) and all(r.mask in (0, iref.BLUR) for r in rows)


def test_philox_known_answers():
    """Random123's known-answer vectors of Philox4x32-10"""
    z = iref.philox4x32_10(np.zeros((1, 4), dtype=np.uint32), (0, 0))[0]
    assert [int(v) for v in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = iref.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, dtype=np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [int(v) for v in f] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    w = iref.noise_words(0x0123456789ABCDEF, 5, first=2 ** 32 - 2)                   # the counter carries into its second word
    assert w.dtype == np.uint32 and w.shape == (5, 4) and len({tuple(r) for r in w.tolist()}) == 5
    u = iref.uniforms(np.array([0, 255, 256, 0xFFFFFFFF], dtype=np.uint32))
    assert u[0] == u[1] == 2.0 ** -25 and u[2] == 1.5 * 2.0 ** -24 and u[3] == 1.0


@pytest.mark.parametrize("sigma", [0.5, 0.62, 1.0, 2.0])
def test_restated_blur_is_scipy_gaussian_filter(sigma):
    x = np.random.default_rng(11).standard_normal((9, 18, 37))
    want = ndi.gaussian_filter(x, float(np.float32(sigma)), mode="reflect", truncate=4.0)
    got = iref.blur(x, np.float32(sigma))
    assert np.abs(got - want).max() <= 1e-14 * np.abs(x).max()


@pytest.mark.parametrize("g", [0.7, 1.5])
@pytest.mark.parametrize("invert", [False, True])
def test_restated_gamma_retains_mean_and_std(g, invert):
    """mean and std come back to 1e-12 relative.  The formula divides by std(y) + 1e-8, so the std comes back times
    std(y) / (std(y) + 1e-8): that factor is within 1e-12 of 1 for the HU-scaled volume (std 3e5, checked against the
    input's std itself) and is accounted for on the z-score-like one (std 3, where it is 1 - 3.8e-9)."""
    z = np.random.default_rng(12).standard_normal((8, 9, 10)) * 3.0 + 1.0
    for x in (z * 1e5, z):
        y = iref.gamma(x, g, invert)
        v = -x if invert else x
        sy = (np.power((v - v.min()) / (v.max() - v.min() + 1e-7), g) * (v.max() - v.min()) + v.min()).std()
        shrink = 1.0 if x is not z else sy / (sy + 1e-8)
        assert abs(y.mean() - x.mean()) <= 1e-12 * abs(x.mean()) and abs(y.std() - x.std() * shrink) <= 1e-12 * x.std()
        assert np.abs(y - x).max() > 1e-3
    c = np.full((8, 8, 8), 0.375)                          # sums of a dyadic constant are exact: the constant itself comes back
    assert np.array_equal(iref.gamma(c, g, invert), c)
    c = np.full((8, 8, 8), -0.37)                          # otherwise numpy's mean of the constant, an ulp from it at most
    assert np.abs(iref.gamma(c, g, invert) - c).max() <= 2.0 ** -52 * 0.37


def test_restated_contrast_keeps_the_range():
    x = np.random.default_rng(13).random((8, 9, 10))
    for f in (0.75, 1.25):
        y = iref.contrast(x, f)
        assert y.min() >= x.min() and y.max() <= x.max() and np.abs(y - x).max() > 1e-3


def test_row_layout_matches_the_header():
    text = open(os.path.join(ROOT, "include", "msseg.h")).read()
    m = re.search(r"/\* (\d+) bytes; offsets: ([^*]+)\*/\s*typedef struct msseg_intensity_row", text)
    assert m, "include/msseg.h states the layout of msseg_intensity_row"
    assert ctypes.sizeof(IntensityRow) == int(m.group(1)) == 32
    stated = {name: int(off) for name, off in re.findall(r"(\w+) (\d+)", m.group(2))}
    assert stated == {name: getattr(IntensityRow, name).offset for name, _ in IntensityRow._fields_}
    assert stated == {"mask": 0, "noise_std": 4, "noise_key": 8, "blur_sigma": 16, "contrast": 20, "gamma_inv": 24, "gamma": 28}
    bits = {n: int(v) for n, v in re.findall(r"#define MSSEG_INTENSITY_(\w+) (\d+)u", text)}
    assert bits == {"NOISE": iref.NOISE, "BLUR": iref.BLUR, "CONTRAST": iref.CONTRAST, "GAMMA_INV": iref.GAMMA_INV,
                    "GAMMA": iref.GAMMA}
