"""Host side of the class-ratio crop centres (--t_rand_crop_class_ratios / --t_rand_crop_center_dilation): flag parsing and
refusals, crop_mode, the per-patch draws of draw_class_rows, and the restatement's dilation against the definition."""
import numpy as np
import pytest

from tests import class_crop_ref as ref

CFG = dict(flip_prob=0.5, rot_prob=0.5, shift_os=0.1, shift_prob=0.5, scale_f=0.1, scale_prob=0.5)


def _args(*flags):
    from medicalsemseg_amd.utils.arguments import get_args
    return get_args(list(flags))


def test_flags_parse_and_default_to_off():
    from medicalsemseg_amd.data_device import check_transform_flags, class_crop_config_from_args
    cfg = _args()
    assert cfg.t_rand_crop_class_ratios == () and cfg.t_rand_crop_center_dilation == 0
    assert class_crop_config_from_args(cfg) == (None, 0)
    check_transform_flags(cfg)
    cfg = _args("--output_dim", "4", "--t_rand_crop_class_ratios", "0.2", "1", "1", "1", "--t_rand_crop_center_dilation", "48")
    assert class_crop_config_from_args(cfg) == ((0.2, 1.0, 1.0, 1.0), 48)
    check_transform_flags(cfg)
    # one class: the parser collapses a list of one value to a scalar
    assert class_crop_config_from_args(_args("--output_dim", "1", "--t_rand_crop_class_ratios", "2")) == ((2.0,), 0)
    assert class_crop_config_from_args(_args("--output_dim", "16", "--t_rand_crop_class_ratios", *["1"] * 16))[0] == (1.0,) * 16
    assert class_crop_config_from_args(_args("--t_rand_crop_class_ratios", "0", "0", "1", "--t_rand_crop_center_dilation",
                                             "254")) == ((0.0, 0.0, 1.0), 254)


@pytest.mark.parametrize("flags", [
    ("--output_dim", "3", "--t_rand_crop_class_ratios", "1", "1"),                       # not output_dim values
    ("--output_dim", "3", "--t_rand_crop_class_ratios", "1", "1", "1", "1"),
    ("--output_dim", "17", "--t_rand_crop_class_ratios", *["1"] * 17),                   # more than 16 classes
    ("--t_rand_crop_class_ratios", "1", "-0.5", "1"),
    ("--t_rand_crop_class_ratios", "1", "nan", "1"),
    ("--t_rand_crop_class_ratios", "1", "inf", "1"),
    ("--t_rand_crop_class_ratios", "0", "0", "0"),
])
def test_bad_ratios_are_a_value_error_that_names_the_flag(flags):
    from medicalsemseg_amd.data_device import check_transform_flags, crop_mode
    with pytest.raises(ValueError, match="--t_rand_crop_class_ratios"):
        check_transform_flags(_args(*flags))
    with pytest.raises(ValueError, match="--t_rand_crop_class_ratios"):
        crop_mode(_args(*flags))


def test_dilation_range_and_dependence_on_the_ratios():
    from medicalsemseg_amd.data_device import check_transform_flags
    for n in ("-1", "255", "1000"):
        with pytest.raises(ValueError, match="--t_rand_crop_center_dilation"):
            check_transform_flags(_args("--t_rand_crop_class_ratios", "1", "1", "1", "--t_rand_crop_center_dilation", n))
    for other in ((), ("--t_rand_crop_fgbg",), ("--t_rand_spatial_crop",)):
        with pytest.raises(ValueError, match="--t_rand_crop_center_dilation.*--t_rand_crop_class_ratios"):
            check_transform_flags(_args("--t_rand_crop_center_dilation", "3", *other))


@pytest.mark.parametrize("other", ["t_rand_crop_fgbg", "t_rand_spatial_crop"])
def test_two_crop_flags_are_an_error_that_names_both(other):
    from medicalsemseg_amd.data_device import crop_mode
    with pytest.raises(ValueError) as e:
        crop_mode(_args("--t_rand_crop_class_ratios", "1", "1", "1", "--" + other))
    assert "--t_rand_crop_class_ratios" in str(e.value) and "--" + other in str(e.value)


def test_reference_flags_stay_refused_and_point_to_the_new_ones():
    from medicalsemseg_amd.data_device import check_transform_flags
    with pytest.raises(NotImplementedError) as e:
        check_transform_flags(_args("--t_rand_crop_classes"))
    assert "t_rand_crop_classes" in str(e.value) and "--t_rand_crop_class_ratios NEG POS POS" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        check_transform_flags(_args("--t_rand_crop_dilated_center"))
    assert "t_rand_crop_dilated_center" in str(e.value) and "--t_rand_crop_center_dilation 48" in str(e.value)
    assert "--t_rand_crop_class_ratios" in str(e.value)
    # also next to valid new flags
    with pytest.raises(NotImplementedError, match="t_rand_crop_classes"):
        check_transform_flags(_args("--t_rand_crop_classes", "--t_rand_crop_class_ratios", "1", "1", "1"))


def test_crop_mode_results():
    from medicalsemseg_amd.data_device import crop_mode
    assert crop_mode(_args("--t_rand_crop_class_ratios", "1", "1", "1")) == "class_ratios"
    assert crop_mode(_args("--t_rand_crop_class_ratios", "1", "1", "1", "--t_rand_crop_center_dilation", "5")) == "class_ratios"
    assert crop_mode(_args("--t_rand_crop_fgbg")) == "fgbg"
    assert crop_mode(_args("--t_rand_spatial_crop")) == "spatial"
    with pytest.raises(SystemExit) as e:
        crop_mode(_args())
    msg = str(e.value)
    old = ("training on files needs a crop flag: --t_rand_crop_fgbg, --t_rand_spatial_crop or --t_rand_crop_classes "
           "(the last one is not implemented on the device data path)")
    assert msg.startswith(old) and "--t_rand_crop_class_ratios" in msg[len(old):]


def test_loader_refuses_inconsistent_arguments_before_touching_the_gpu():
    """class_ratios and crop="class_ratios" go together; bad ratios and dilations are refused by the constructor too"""
    from medicalsemseg_amd.data_device import DeviceDatasetLoader, class_crop_config
    vols = [{"img": None, "lab": None}]
    with pytest.raises(ValueError, match="class_ratios"):
        DeviceDatasetLoader(vols, 16, 1, 1, crop="class_ratios")
    with pytest.raises(ValueError, match="class_ratios"):
        DeviceDatasetLoader(vols, 16, 1, 1, crop="fgbg", class_ratios=(1, 1))
    with pytest.raises(ValueError, match="t_rand_crop_center_dilation"):
        DeviceDatasetLoader(vols, 16, 1, 1, crop="class_ratios", class_ratios=(1, 1), center_dilation=255)
    with pytest.raises(ValueError, match="t_rand_crop_center_dilation"):
        DeviceDatasetLoader(vols, 16, 1, 1, crop="fgbg", center_dilation=2)
    with pytest.raises(ValueError, match="t_rand_crop_class_ratios"):
        class_crop_config((1.0,) * 17)
    assert class_crop_config(None) == (None, 0) and class_crop_config((0, 3), 7) == ((0.0, 3.0), 7)


def test_draw_class_rows_frequencies_follow_the_ratios():
    """ratios (1, 1, 2), all counts positive, 4000 draws: every class frequency within 0.04 of its ratio -- 5 sigma of a
    binomial with p = 1/2, n = 4000 (sigma = 0.0079), wider than 5 sigma of the p = 1/4 classes"""
    from medicalsemseg_amd.data_device import draw_class_rows
    counts = (1000, 7, 300)
    rows = draw_class_rows(np.random.default_rng(5), 4000, counts, (1.0, 1.0, 2.0), CFG)
    cls = np.array([r[0] for r in rows])
    freq = np.bincount(cls, minlength=3) / 4000.0
    print("class frequencies", freq)
    assert np.all(np.abs(freq - np.array([0.25, 0.25, 0.5])) <= 0.04)
    for c, idx, flips, rotk, shift, scale in rows:
        assert 0 <= idx < counts[c] and len(flips) == 3 and 0 <= rotk <= 3 and abs(shift) <= 0.1 and abs(scale - 1.0) <= 0.1
    # every candidate of the small class is reached, the index is uniform over the class's own list
    assert {r[1] for r in rows if r[0] == 1} == set(range(7))
    # seeded: the same generator state gives the same rows
    assert rows[:50] == draw_class_rows(np.random.default_rng(5), 50, counts, (1.0, 1.0, 2.0), CFG)


def test_draw_class_rows_drops_empty_classes_and_renormalises():
    from medicalsemseg_amd.data_device import draw_class_rows
    rows = draw_class_rows(np.random.default_rng(6), 4000, (50, 0, 20, 0), (1.0, 5.0, 1.0, 3.0), CFG)
    cls = np.array([r[0] for r in rows])
    assert set(cls.tolist()) == {0, 2}
    freq = np.bincount(cls, minlength=4) / 4000.0
    assert abs(freq[0] - 0.5) <= 0.04 and abs(freq[2] - 0.5) <= 0.04
    # a ratio of 0 is never drawn either, whatever its count; a single live class takes every draw
    rows = draw_class_rows(np.random.default_rng(7), 500, (50, 60, 20), (0.0, 0.0, 1.0), CFG)
    assert {r[0] for r in rows} == {2}
    rows = draw_class_rows(np.random.default_rng(7), 500, (50, 60, 20), (0.0, 1.0, 0.0), CFG)
    assert {r[0] for r in rows} == {1}


def test_draw_class_rows_without_any_candidate_falls_back_to_a_voxel():
    from medicalsemseg_amd.data_device import draw_class_rows
    for counts, ratios in (((0, 0, 0), (1.0, 1.0, 1.0)), ((5, 0, 0), (0.0, 1.0, 1.0))):
        rows = draw_class_rows(np.random.default_rng(8), 20, counts, ratios, CFG)
        assert all(r[0] == -1 and r[1] == 0 for r in rows)
        assert len({r[2:] for r in rows}) > 1                    # the other draws are still made


@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_restated_dilation_equals_the_l1_definition(n):
    rng = np.random.default_rng(9)
    mask = rng.random((6, 7, 8)) < 0.02
    mask[0, 0, 0] = True
    assert np.array_equal(ref.dilate(mask, n), ref.dilate_brute(mask, n))
    assert not ref.dilate(np.zeros((6, 7, 8), bool), n).any()
    # the candidate sets: the image rule applies to every class, labels >= K to none
    lab = rng.integers(0, 5, (6, 7, 8)).astype(np.uint8)
    img = rng.standard_normal((6, 7, 8)).astype(np.float32)
    got = ref.candidate_mask(img, lab, (0, 2), n, 0.0, "gt")
    assert np.array_equal((got >> 2) & 1, ref.dilate_brute(lab == 2, n) & (img > 0))
    assert not (got & ~np.uint16(0b101)).any()
    assert np.array_equal(ref.slab_counts(img, lab, 3, n, classes=(0, 2))[:, 2], ((got >> 2) & 1).reshape(6, -1).sum(1))
