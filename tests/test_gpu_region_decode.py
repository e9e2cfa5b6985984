"""GPU tests of the inference side of region-based training (--label_regions): msseg_region_decode_u8 and
msseg_region_counts_u8 bit for bit against numpy (tests/region_ref.py), engine.test.label_map with a table, the refusal of
--restore_mode linear, and run_score.py's region rows against metrics.surface_metrics on the table-mapped maps."""
import json
import os

import numpy as np
import pytest
import torch

from tests import region_ref as rr
from tests import surface_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 210 and 5049 voxels (no multiple of 4: one voxel per thread, one block and several); 336: four voxels per thread
SHAPES = [(5, 6, 7), (33, 17, 9), (8, 6, 7)]
VALUES = {1: (7,), 3: (1, 2, 3), 16: (1, 2, 3, 0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 255, 200)}


def _logits(C, shape, seed):
    """integer-valued logits in -2..2 (exact zeros, which must not fire) with a few NaNs"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (C, *shape)).astype(np.float32)
    x.reshape(-1)[rng.choice(x.size, 5, replace=False)] = np.nan
    assert (x == 0).any() and np.isnan(x).any()
    return x


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", [1, 3, 16])
def test_region_decode_u8(C, shape):
    from medicalsemseg_amd import hip
    x = _logits(C, shape, 10 * C + shape[0])
    want_map, want_bits = rr.decode(x.reshape(C, -1), VALUES[C])
    t = torch.from_numpy(x).to(DEV)
    got, bits = hip.region_decode_u8(t, VALUES[C], want_bits=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape and bits.dtype == torch.uint16
    assert np.array_equal(got.cpu().numpy().reshape(-1), want_map)
    assert np.array_equal(bits.cpu().numpy().reshape(-1), want_bits)
    alone = hip.region_decode_u8(t, VALUES[C])                                  # bits == NULL
    assert torch.equal(alone, got)
    if C == 16:
        assert want_bits.max() >= 1 << 15 and (want_map == 200).any() and (want_map == 255).any()


def test_region_decode_refusals():
    from medicalsemseg_amd import hip
    t = torch.zeros(3, 2, 2, 2, device=DEV)
    with pytest.raises(ValueError, match="region_decode_u8"):
        hip.region_decode_u8(t, (1, 2))
    with pytest.raises(ValueError, match="region_decode_u8"):
        hip.region_decode_u8(t, (1, 2, 256))
    out = torch.zeros(8, dtype=torch.uint8, device=DEV)
    for C in (0, 17):
        assert hip.lib().msseg_region_decode_u8(t.data_ptr(), C, 8, (hip.C.c_uint8 * 16)(), out.data_ptr(), None, None) == -1
        assert hip.lib().msseg_region_counts_u8(out.data_ptr(), out.data_ptr(), 8, C, hip.region_masks((1,)), t.data_ptr(),
                                                None, 0, None) == -1


@pytest.mark.parametrize("shape", SHAPES)
def test_region_counts_u8(shape):
    from medicalsemseg_amd import hip
    rng = np.random.default_rng(shape[0])
    pred = rng.integers(0, 4, shape).astype(np.uint8)
    label = rng.integers(0, 4, shape).astype(np.uint8)
    label.reshape(-1)[:3] = (31, 40, 255)                                       # in no region of the table
    masks = rr.BRAIN_TUMOUR[0]
    got = hip.region_counts_u8(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), masks)
    again = hip.region_counts_u8(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), masks)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 3) and torch.equal(got, again)
    assert np.array_equal(got.double().cpu().numpy(), rr.counts(pred, label, masks))


def test_label_map_and_dice_of_maps_with_a_table():
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.engine.test import dice_of_maps, label_map
    x = torch.from_numpy(_logits(3, (33, 17, 9), 3)).to(DEV)
    table = rr.BRAIN_TUMOUR
    seg = label_map(x[None], table)
    assert torch.equal(seg, hip.region_decode_u8(x, table[1]))
    assert torch.equal(label_map(x[None].nan_to_num(0.0)), hip.argmax_u8(x.nan_to_num(0.0)))    # without one: the arg max
    rng = np.random.default_rng(4)
    label = rng.integers(0, 4, (1, 1, 33, 17, 9)).astype(np.uint8)
    c = rr.counts(seg.cpu().numpy(), label, table[0])
    want = float(np.mean(2.0 * c[:, 0] / (c[:, 1] + c[:, 2])))
    got = dice_of_maps(seg[None], torch.from_numpy(label).to(DEV).float(), 3, table)
    assert abs(got - want) < 1e-6, (got, want)


def test_linear_restore_is_refused_under_regions():
    from medicalsemseg_amd.data import SyntheticLoader
    from medicalsemseg_amd.engine.test import test_model
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.utils.arguments import get_args
    cfg = get_args("--model UNetSmall --output_dim 2 --label_regions 1,2=1 2=2 --vol_size 16 --restore_mode linear".split())
    model = build_model(cfg).to(DEV)
    with pytest.raises(ValueError, match="--label_regions") as e:
        test_model(model, SyntheticLoader(1, 1, 16, 1, 3, seed=2, with_crop_info=False), torch.device(DEV), cfg)
    assert "--restore_mode linear" in str(e.value)


def _nested_spheres(shape=(24, 24, 24)):
    xx, yy, zz = np.ogrid[:shape[0], :shape[1], :shape[2]]
    r2 = (xx - 11.5) ** 2 + (yy - 11.5) ** 2 + (zz - 11.5) ** 2
    lab = np.zeros(shape, np.uint8)
    lab[r2 <= 9.0 ** 2] = 1
    lab[r2 <= 5.0 ** 2] = 2
    return lab


def test_run_score_region_rows(tmp_path):
    """24^3, two nested spheres (labels 1 and 2), regions 1,2 and 2: run_score.py's rows equal metrics.surface_metrics(.., 2, ..)
    class 1 on the table-mapped maps and the Dice of the numpy counts"""
    import run_score
    from medicalsemseg_amd import data_files, metrics
    from medicalsemseg_amd.utils.nifti import load_nifti
    lab = _nested_spheres()
    pred = np.roll(lab, (1, -1, 2), (0, 1, 2))
    data_path, task, pdir = sr.write_score_task(tmp_path, {"000": lab}, {"000": pred})
    out = os.path.join(str(tmp_path), "scores.json")
    tau = [1.0, 2.0]
    run_score.main(run_score.build_parser().parse_args(
        ["--pred_folder", pdir, "--data_path", data_path, "--task", task, "--label_regions", "1,2=1", "2=2", "--nsd_tolerance",
         *[str(t) for t in tau], "--out", out]))
    with open(out) as f:
        js = json.load(f)
    case = js["cases"]["000.nii.gz"]
    assert js["n_classes"] == 2 and js["label_regions"] == ["1,2=1", "2=2"]
    assert [r["region"] for r in js["summary"]["per_class"]] == [0, 1] and js["summary"]["foreground"]["n_cases"] == 1
    pr, aff = load_nifti(os.path.join(pdir, "000.nii.gz"))
    gt, _ = load_nifti(os.path.join(data_path, task, "labelsTr", "000.nii.gz"))
    spacing = data_files.spacing_of(aff)
    masks = (0b110, 0b100)
    c = rr.counts(pr, gt, masks)
    for r, m in enumerate(masks):
        t = rr.lut(m)
        a, b = (torch.from_numpy(np.ascontiguousarray(t[v.astype(np.uint8)])).to(DEV) for v in (pr, gt))
        want = metrics.surface_metrics(a, b, 2, spacing, [tau[r]])
        for k in ("hd_mm", "assd_mm", "nsd"):
            assert case[k][r] == float(want[k][1]) and np.isfinite(case[k][r]), (k, r, case[k], want[k])
        assert abs(case["dice"][r] - 2.0 * c[r, 0] / (c[r, 1] + c[r, 2])) < 1e-6
    assert js["summary"]["per_class"][1]["hd_mm"] == case["hd_mm"][1]
    assert js["summary"]["foreground"]["dice"] == pytest.approx(np.mean(case["dice"]), rel=1e-12)
