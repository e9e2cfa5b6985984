"""msseg_restore_native_u8 (csrc/restore.hip) and the file driver run_predict.py on the GPU.  Every comparison with
tests/restore_ref.py is exact equality of uint8 maps: both sides do the same IEEE operations in the same order."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import restore_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = (20, 37, 29)            # three distinct lengths, axis 2 no multiple of 4, more than one block on every axis


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _ctypes_desc(desc):
    from medicalsemseg_amd import hip
    d = hip.RestoreDesc()
    for k in range(3):
        for f in rr.FIELDS:
            getattr(d, f)[k] = desc[f][k]
    return d


def _cropped_desc(native, perm, flip, scale=(1.0, 1.0, 1.0), lo=(2, 3, 1), cut_hi=(2, 1, 3), pad_axis=1, pad_before=2, pad_extra=5):
    """the descriptor of: orientation -> spacing (grid by resample_shape's rule) -> a crop box strictly inside the grid ->
    a pad on one axis, the model grid larger than the box there"""
    n = [native[p] for p in perm]
    grid = tuple(max(int(np.round((n[k] - 1) * float(scale[k]) + 1.0)), 1) for k in range(3))
    hi = tuple(grid[k] - cut_hi[k] for k in range(3))
    assert all(0 < lo[k] < hi[k] < grid[k] for k in range(3))
    model = [hi[k] - lo[k] for k in range(3)]
    before = [0, 0, 0]
    model[pad_axis] += pad_extra
    before[pad_axis] = pad_before
    return rr.make_desc(native, perm, flip, grid, tuple(before[k] - lo[k] for k in range(3)), tuple(model), scale)


@pytest.mark.parametrize("perm,flip", rr.ORIENTATIONS)
def test_nearest_every_orientation(perm, flip):
    from medicalsemseg_amd import hip
    desc = _cropped_desc(NATIVE, perm, flip)
    lab = np.random.default_rng(11).integers(1, 250, size=desc["model"], dtype=np.uint8)
    got = hip.restore_native_u8(torch.from_numpy(lab).to(_dev()), _ctypes_desc(desc), "nearest")
    assert got.dtype == torch.uint8 and tuple(got.shape) == NATIVE and got.is_contiguous()
    want = rr.restore_ref(lab, desc, "nearest")
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(want, rr.restore_by_construction(lab, desc))


# the two spacing cases: (scale, what the case must exercise)
SPACING = [((1.5, 0.8, 1.0), "clamp"), ((0.5, 1.25, 2.0), None)]


def _spacing_desc(scale):
    # oriented lengths (29, 20, 37); the box starts at ceil(1 * scale[0]) on axis 0, so that native index 1 of that axis
    # lands half a voxel in front of the model grid
    lo0 = int(np.ceil(scale[0]))
    return _cropped_desc(NATIVE, (2, 0, 1), (1, 0, 1), scale, lo=(lo0, 3, 1), pad_axis=1)


@pytest.mark.parametrize("scale,must", SPACING)
def test_spacing_cases_are_what_they_claim(scale, must):
    """host-side: the tap clamp (m in [-0.5, 0)) runs in both cases, the half-voxel clamp (s > grid - 1) in the first, and
    both on voxels that lie on the model grid along every axis, where they change the output and are not zeroed as air"""
    desc = _spacing_desc(scale)
    m = [rr.axis_coords(desc, k) for k in range(3)]
    on_grid = [(np.floor(m[k] + 0.5) >= 0) & (np.floor(m[k] + 0.5) < desc["model"][k]) for k in range(3)]
    assert all(g.any() for g in on_grid)
    assert (((m[0] >= -0.5) & (m[0] < 0.0)) & on_grid[0]).any()
    clamped = []
    for k in range(3):
        n = desc["native"][desc["perm"][k]]
        o = np.arange(n) if not desc["flip"][k] else n - 1 - np.arange(n)
        clamped.append(bool(((o * desc["scale"][k] > desc["grid"][k] - 1) & on_grid[k]).any()))
    assert any(clamped) == (must == "clamp")


@pytest.fixture(scope="module")
def spacing_logits():
    """per (scale, C, kind) the logits on the host, made once"""
    out = {}
    for scale, _ in SPACING:
        model = _spacing_desc(scale)["model"]
        for C in (2, 5):
            rng = np.random.default_rng(100 + C)
            out[scale, C, "int"] = rng.integers(-4, 5, size=(C,) + model).astype(np.float32)
            out[scale, C, "gauss"] = rng.normal(0.0, 1.0, size=(C,) + model).astype(np.float32)
    return out


@pytest.mark.parametrize("scale,must", SPACING)
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_spacing_linear(scale, must, C, kind, spacing_logits):
    from medicalsemseg_amd import hip
    desc = _spacing_desc(scale)
    logits = spacing_logits[scale, C, kind]
    got = hip.restore_native_u8(torch.from_numpy(logits).to(_dev()), _ctypes_desc(desc), "linear").cpu().numpy()
    want = rr.restore_ref(logits, desc, "linear")
    assert got.shape == NATIVE and np.array_equal(got, want)
    assert len(np.unique(want)) == C                                 # every class wins somewhere: the case is not trivial


@pytest.mark.parametrize("scale,must", SPACING)
def test_spacing_nearest(scale, must):
    from medicalsemseg_amd import hip
    desc = _spacing_desc(scale)
    lab = np.random.default_rng(12).integers(1, 250, size=desc["model"], dtype=np.uint8)
    got = hip.restore_native_u8(torch.from_numpy(lab).to(_dev()), _ctypes_desc(desc), "nearest").cpu().numpy()
    assert np.array_equal(got, rr.restore_ref(lab, desc, "nearest"))


def test_identity_descriptor():
    from medicalsemseg_amd import hip
    dev = _dev()
    rng = np.random.default_rng(13)
    desc = _ctypes_desc(rr.make_desc(NATIVE))
    logits = torch.from_numpy(rng.integers(-3, 4, size=(5,) + NATIVE).astype(np.float32)).to(dev)   # ties: first maximum
    assert torch.equal(hip.restore_native_u8(logits, desc, "linear"), hip.argmax_u8(logits))
    gauss = torch.from_numpy(rng.normal(size=(3,) + NATIVE).astype(np.float32)).to(dev)
    assert torch.equal(hip.restore_native_u8(gauss, desc, "linear"), hip.argmax_u8(gauss))
    lab = torch.from_numpy(rng.integers(0, 255, size=NATIVE, dtype=np.uint8)).to(dev)
    assert torch.equal(hip.restore_native_u8(lab, desc, "nearest"), lab)


def test_round_trip_through_preprocess_volume():
    """LPS file -> RAS, foreground crop, pad (no spacing) -> back: the label inside the foreground box, 0 elsewhere"""
    from medicalsemseg_amd import hip
    from medicalsemseg_amd.data_device import preprocess_volume
    from medicalsemseg_amd.utils.arguments import get_args
    rng = np.random.default_rng(14)
    shape = (40, 28, 36)
    img = np.zeros((1,) + shape, dtype=np.float32)
    img[:, 5:33, 3:24, 6:30] = rng.uniform(0.5, 1.0, size=(1, 28, 21, 24)).astype(np.float32)
    lab = rng.integers(0, 4, size=shape, dtype=np.uint8)            # labels outside the box too: they must come back as 0
    aff = np.diag([-1.0, -1.0, 1.0, 1.0])
    aff[:3, 3] = (12.0, -7.0, 3.0)
    cfg = get_args(["--vol_size", "32", "--t_crop_foreground_img", "--t_spatial_pad"])
    rec = preprocess_volume(img, lab, aff, cfg, _dev(), "lps.nii.gz")
    perm, flips = rec["orient"]
    assert (perm, flips) == ((0, 1, 2), (True, True, False)) and rec["native_shape"] == shape
    assert rec["spacing_scale"] == (1.0, 1.0, 1.0) and rec["grid_shape"] == shape
    assert max(rec["pad_before"]) > 0 and tuple(rec["lab"].shape) == rec["model_shape"]
    got = hip.restore_native_u8(rec["lab"], rec).cpu().numpy()
    box = rec["box"]
    sl = [None] * 3
    for k in range(3):                                               # the box on the native axes
        n, lo, hi = shape[perm[k]], box[k], box[3 + k]
        sl[perm[k]] = slice(n - hi, n - lo) if flips[k] else slice(lo, hi)
    assert tuple((s.start, s.stop) for s in sl) == ((5, 33), (3, 24), (6, 30))
    want = np.zeros(shape, dtype=np.uint8)
    want[tuple(sl)] = lab[tuple(sl)]
    assert np.array_equal(got, want)


def test_linear_mode_allocates_the_output_only():
    """C = 5 on native (48, 40, 56): the unfused route would hold [C][native] fp32 = 2.1 MB"""
    from medicalsemseg_amd import hip
    dev = _dev()
    native = (48, 40, 56)
    desc = _ctypes_desc(_cropped_desc(native, (1, 2, 0), (0, 1, 1), (1.5, 0.8, 1.25)))
    logits = torch.randn((5,) + tuple(desc.model), device=dev)
    hip.restore_native_u8(logits, desc, "linear")                    # the library is loaded, the code object is resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.max_memory_allocated(dev)
    out = hip.restore_native_u8(logits, desc, "linear")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    assert tuple(out.shape) == native
    assert rise <= int(np.prod(native)) + 64 * 1024, rise


@pytest.mark.parametrize("what", ["perm", "zero_dim", "nan_scale", "c_zero", "long_axis"])
def test_invalid_descriptors_launch_nothing(what):
    from medicalsemseg_amd import hip
    dev = _dev()
    # long_axis: native axes 0 and 1 come from the launch grid, which holds 65535 blocks along each
    native = (3, 65536, 4) if what == "long_axis" else NATIVE
    desc = rr.make_desc(native)
    logits_mode, C = what == "c_zero", 0
    if what == "perm":
        desc["perm"] = (0, 2, 2)
    elif what == "zero_dim":
        desc["grid"] = (NATIVE[0], 0, NATIVE[2])
    elif what == "nan_scale":
        desc["scale"] = (1.0, float("nan"), 1.0)
    d = _ctypes_desc(desc)
    src = torch.zeros((5,) + native, dtype=torch.float32, device=dev) if logits_mode else \
        torch.ones(native, dtype=torch.uint8, device=dev)
    dst = torch.full(native, 0xAB, dtype=torch.uint8, device=dev)
    rc = hip.lib().msseg_restore_native_u8(src.data_ptr(), int(logits_mode), C, ctypes.addressof(d), dst.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1                                                   # MSSEG_EINVAL
    assert bool((dst == 0xAB).all())
    with pytest.raises(hip.MssegError, match="restore_native_u8"):
        hip.restore_native_u8(src[:0] if logits_mode else src, d, "linear" if logits_mode else "nearest")


def test_binding_refuses_cpu_dtype_and_shape():
    from medicalsemseg_amd import hip
    d = _ctypes_desc(rr.make_desc(NATIVE))
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.restore_native_u8(torch.zeros(NATIVE, dtype=torch.uint8), d)
    dev = _dev()
    with pytest.raises(AssertionError):
        hip.restore_native_u8(torch.zeros(NATIVE, dtype=torch.float32, device=dev), d, "nearest")
    with pytest.raises(AssertionError):
        hip.restore_native_u8(torch.zeros((2,) + NATIVE, dtype=torch.float32, device=dev).transpose(2, 3), d, "linear")
    with pytest.raises(ValueError, match="grid"):
        hip.restore_native_u8(torch.zeros((20, 37, 28), dtype=torch.uint8, device=dev), d)
    with pytest.raises(ValueError, match="mode"):
        hip.restore_native_u8(torch.zeros(NATIVE, dtype=torch.uint8, device=dev), d, "cubic")


# ---- run_predict.py, majority_vote.py -------------------------------------------------------------------------------
DRIVER_FLAGS = ["--model", "UNetSmall", "--output_dim", "3", "--vol_size", "32", "--t_voxel_spacings", "--t_voxel_dims", "1.5",
                "--t_crop_foreground_img", "--t_spatial_pad", "--save_eval_output", "--task", "Task98_Files",
                "--json_list", "dataset.json"]
CASES = {  # name -> (shape, affine diagonal, translation, foreground block)
    "case_lps.nii.gz": ((40, 52, 44), (-1.5, -1.0, 2.0), (31.0, -12.0, 5.0), (slice(4, 37), slice(6, 47), slice(3, 40))),
    "case_ras.nii.gz": ((36, 30, 40), (1.5, 1.5, 1.5), (-3.0, 8.0, 2.5), (slice(3, 33), slice(2, 20), slice(5, 36))),
}


@pytest.fixture(scope="module")
def file_task(tmp_path_factory):
    """two tiny NIfTI files with a data list that has a "test" section, and two checkpoints of the smallest UNet"""
    from medicalsemseg_amd.models.model_builder import build_model
    from medicalsemseg_amd.utils.arguments import get_args
    from medicalsemseg_amd.utils.nifti import save_nifti
    root = tmp_path_factory.mktemp("files")
    task = root / "data" / "Task98_Files"
    os.makedirs(task / "imagesTs")
    rng = np.random.default_rng(15)
    for name, (shape, diag, trans, block) in CASES.items():
        img = np.zeros(shape, dtype=np.float32)
        img[block] = rng.uniform(0.2, 1.0, size=img[block].shape).astype(np.float32)
        aff = np.diag(diag + (1.0,))
        aff[:3, 3] = trans
        save_nifti(str(task / "imagesTs" / name), img, aff)
    with open(task / "dataset.json", "w") as f:
        json.dump({"test": ["./imagesTs/" + n for n in CASES]}, f)
    cks = []
    for fold in range(2):
        torch.manual_seed(40 + fold)
        model = build_model(get_args(DRIVER_FLAGS))
        cks.append(str(root / f"fold{fold}.pth"))
        torch.save({"model": model.state_dict()}, cks[-1])
    return str(root / "data"), cks, root


def _run_predict(data_path, ck, out, fold, mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_predict.py"), *DRIVER_FLAGS, "--data_path", data_path, "--resume", ck,
                        "--output_dir", out, "--cv_fold", str(fold), "--restore_mode", mode],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def _rebuilt_desc(name, data_path, pred_shape):
    """the descriptor of a case, put together here: orientation and spacing from what the file was written with, the grid
    by the spacing rule, the model grid from the saved pred/ map; only the foreground box and the pad come from a
    preprocess_volume run of the same flags (they are existing keys, pinned by the data tests)"""
    from medicalsemseg_amd.data_device import preprocess_volume, restore_descriptor
    from medicalsemseg_amd.utils.arguments import get_args
    from medicalsemseg_amd.utils.nifti import load_nifti
    shape, diag, _, _ = CASES[name]
    img, aff = load_nifti(os.path.join(data_path, "Task98_Files", "imagesTs", name))
    rec = preprocess_volume(img[None], None, aff, get_args(DRIVER_FLAGS), _dev(), name)
    scale = tuple(float(abs(d)) / 1.5 for d in diag)
    grid = tuple(max(int(np.round((shape[k] - 1) * abs(diag[k]) / 1.5 + 1.0)), 1) for k in range(3))
    desc = rr.make_desc(shape, (0, 1, 2), tuple(d < 0 for d in diag), grid,
                        tuple(rec["pad_before"][k] - rec["box"][k] for k in range(3)), pred_shape, scale)
    assert rr.desc_of(restore_descriptor(rec)) == desc               # the record's new keys say the same
    return desc


def test_run_predict_nearest_two_folds_and_vote(file_task):
    from medicalsemseg_amd.utils.nifti import load_nifti
    data_path, cks, root = file_task
    out = str(root / "out_nearest")
    for fold in range(2):
        _run_predict(data_path, cks[fold], out, fold, "nearest")
    for name, (shape, _, _, _) in CASES.items():
        _, file_aff = load_nifti(os.path.join(data_path, "Task98_Files", "imagesTs", name))
        for fold in range(2):
            base = os.path.join(out, "test_output", f"Fold{fold}")
            native, aff = load_nifti(os.path.join(base, "native", name))
            assert native.dtype == np.uint8 and native.shape == shape and np.array_equal(aff, file_aff)
            pred, pred_aff = load_nifti(os.path.join(base, "pred", name))
            assert np.array_equal(pred_aff[:3, 3], np.zeros(3))      # pred/ keeps the reference's zeroed translation
            assert min(pred.shape) >= 32
            desc = _rebuilt_desc(name, data_path, pred.shape)
            assert np.array_equal(native, rr.restore_ref(np.ascontiguousarray(pred), desc, "nearest"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "majority_vote.py"), "--in_folder", os.path.join(out, "test_output"),
                        "--n_classes", "3", "--subfolder_prefix", "native", "--folds", "2"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in CASES:
        folds = [load_nifti(os.path.join(out, "test_output", f"Fold{k}", "native", name)) for k in range(2)]
        voted, aff = load_nifti(os.path.join(out, "test_output", "voted_output", "native", name))
        assert np.array_equal(voted, rr.majority_vote_ref(np.stack([f[0] for f in folds]), 3))
        assert np.array_equal(aff, folds[0][1])


def test_run_predict_linear(file_task):
    from medicalsemseg_amd.utils.nifti import load_nifti
    data_path, cks, root = file_task
    out = str(root / "out_linear")
    _run_predict(data_path, cks[0], out, 0, "linear")
    for name, (shape, _, _, _) in CASES.items():
        _, file_aff = load_nifti(os.path.join(data_path, "Task98_Files", "imagesTs", name))
        base = os.path.join(out, "test_output", "Fold0")
        native, aff = load_nifti(os.path.join(base, "native", name))
        assert native.dtype == np.uint8 and native.shape == shape and np.array_equal(aff, file_aff)
        assert int(native.max()) < 3
        # what the crop removed is air in this mode too (the logits are not saved: the blend itself is pinned above)
        pred, _ = load_nifti(os.path.join(base, "pred", name))
        air = rr.restore_ref(np.ones(pred.shape, dtype=np.uint8), _rebuilt_desc(name, data_path, pred.shape), "nearest") == 0
        assert air.any() and not air.all() and not native[air].any()
