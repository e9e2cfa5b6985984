"""Device-side training patches from volumes cached in HBM.

The reference crops and augments on the CPU with MONAI transforms and ``num_workers = 0``
(``/root/reference/data/dataset_builder.py:108-193``, hand-off ``run_training.py:59-66``); at hundreds of 96^3 patches per
second per GPU that chain is the bottleneck directly in front of the hot path.  Here the whole (normalised) volume and its
label map stay on the device (288 GB of HBM hold hundreds of CT volumes), the random draws of one batch -- crop centre
per patch (foreground / background voxel picked with the reference's pos : neg odds), three flip coins, a quarter-turn
count, intensity shift and scale -- are made on the host with a seeded ``numpy`` generator, and ONE gather kernel
(``msseg_aug_crop_batch``) writes the batch; with ``affine_prob > 0`` a rotation + zoom matrix per patch is drawn as well and
the gather samples the volume under it (``msseg_aug_crop_affine``, still one launch).  ``iter(DevicePatchLoader)`` yields the batch dict the engine consumes,
including the crop centre record the reference's transform fork adds (``data/transforms.py:411``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import hip
from .utils.arguments import n_label_values, region_table


class AugRow(C.Structure):
    """mirror of msseg_aug_row (include/msseg.h)"""
    _fields_ = [("z0", C.c_int32), ("y0", C.c_int32), ("x0", C.c_int32), ("flips", C.c_int32), ("rotk", C.c_int32),
                ("pad0", C.c_int32), ("shift", C.c_float), ("scale", C.c_float)]


def correct_crop_center(center, roi, img_size):
    """keep the roi inside the image (MONAI correct_crop_centers semantics)"""
    out = []
    for c, r, n in zip(center, roi, img_size):
        lo = r // 2
        hi = n + 1 - r / 2.0
        hi = int(np.floor(hi)) if hi == int(hi) else int(np.ceil(hi))
        if lo == hi:
            hi += 1
        c = int(c)
        c = lo if c < lo else c
        c = hi - 1 if c >= hi else c
        out.append(c)
    return tuple(out)


def draw_rows(rng: np.random.Generator, n, fg_count, bg_count, cfg_like):
    """the random draws of n patches: (use_fg, index into the fg/bg voxel list, flips, rotk, shift, scale) per patch"""
    pos, neg = float(cfg_like["pos"]), float(cfg_like["neg"])
    rows = []
    for _ in range(n):
        use_fg = (rng.random() < pos / (pos + neg)) if fg_count > 0 and bg_count > 0 else fg_count > 0
        idx = int(rng.integers(0, fg_count if use_fg else max(bg_count, 1)))
        flips = tuple(bool(rng.random() < cfg_like["flip_prob"]) for _ in range(3))
        rotk = int(rng.integers(1, 4)) if rng.random() < cfg_like["rot_prob"] else 0
        shift = float(rng.uniform(-cfg_like["shift_os"], cfg_like["shift_os"])) if rng.random() < cfg_like["shift_prob"] else 0.0
        scale = 1.0 + (float(rng.uniform(-cfg_like["scale_f"], cfg_like["scale_f"])) if rng.random() < cfg_like["scale_prob"] else 0.0)
        rows.append((use_fg, idx, flips, rotk, shift, scale))
    return rows


def draw_class_rows(rng: np.random.Generator, n, counts, ratios, cfg_like):
    """the random draws of n patches of the class-ratio crop: (class, index into that class's candidate list, flips, rotk,
    shift, scale) per patch.  counts: the volume's candidates per class.  The ratios of the classes without a candidate are
    zeroed and the rest renormalised (MONAI generate_label_classes_crop_centers); one uniform number picks the class by the
    inverse CDF, one integer the candidate; the other draws follow in draw_rows's order.  With no candidate of any class of
    positive ratio the class is -1 and the index 0 (the caller takes a uniform voxel): the uniform number is then not drawn."""
    p = np.array([float(r) if int(c) > 0 else 0.0 for r, c in zip(ratios, counts)], dtype=np.float64)
    live = np.nonzero(p > 0.0)[0]
    cdf = np.cumsum(p / p.sum()) if live.size else None
    rows = []
    for _ in range(n):
        # side="right": a class of probability 0 spans no interval; the last live class also takes a rounded-down total
        cls = min(int(np.searchsorted(cdf, rng.random(), side="right")), int(live[-1])) if live.size else -1
        idx = int(rng.integers(0, int(counts[cls]) if cls >= 0 else 1))
        flips = tuple(bool(rng.random() < cfg_like["flip_prob"]) for _ in range(3))
        rotk = int(rng.integers(1, 4)) if rng.random() < cfg_like["rot_prob"] else 0
        shift = float(rng.uniform(-cfg_like["shift_os"], cfg_like["shift_os"])) if rng.random() < cfg_like["shift_prob"] else 0.0
        scale = 1.0 + (float(rng.uniform(-cfg_like["scale_f"], cfg_like["scale_f"])) if rng.random() < cfg_like["scale_prob"] else 0.0)
        rows.append((cls, idx, flips, rotk, shift, scale))
    return rows


def class_crop_config(ratios, dilation=0, n_classes=None):
    """--t_rand_crop_class_ratios / --t_rand_crop_center_dilation -> (ratios as a tuple of floats, or None when the crop is
    off; dilation); a ValueError names the flag.  n_classes: the number of label values (arguments.n_label_values: --output_dim
    without --label_regions), the number of ratios expected."""
    r = tuple(ratios) if isinstance(ratios, (tuple, list)) else (() if ratios is None else (ratios,))
    n = int(dilation)
    if not 0 <= n <= hip.MAX_CENTER_DILATION:
        raise ValueError(f"--t_rand_crop_center_dilation takes a number of voxels in 0..{hip.MAX_CENTER_DILATION}, got {dilation!r}")
    if not r:
        if n:
            raise ValueError("--t_rand_crop_center_dilation needs --t_rand_crop_class_ratios")
        return None, 0
    want = f"one ratio per class ({n_classes} for --output_dim {n_classes})" if n_classes is not None else "one ratio per class"
    if len(r) > hip.MAX_CROP_CLASSES or (n_classes is not None and len(r) != int(n_classes)):
        raise ValueError(f"--t_rand_crop_class_ratios takes {want}, at most {hip.MAX_CROP_CLASSES}, got {len(r)}: {ratios!r}")
    if not all(np.isfinite(float(v)) and float(v) >= 0.0 for v in r) or not any(float(v) > 0.0 for v in r):
        raise ValueError(f"--t_rand_crop_class_ratios takes finite ratios >= 0 with at least one > 0, got {ratios!r}")
    return tuple(float(v) for v in r), n


def class_crop_config_from_args(cfg):
    """the flags of a parsed command line -> class_crop_config(...); giving the class ratios together with another crop
    flag is a ValueError that names both"""
    ratios, n = class_crop_config(getattr(cfg, "t_rand_crop_class_ratios", ()), getattr(cfg, "t_rand_crop_center_dilation", 0),
                                  n_label_values(cfg) if hasattr(cfg, "output_dim") else None)
    if ratios is not None:
        for other in ("t_rand_crop_fgbg", "t_rand_spatial_crop"):
            if getattr(cfg, other, False):
                raise ValueError(f"--t_rand_crop_class_ratios and --{other} are both crop flags: give one")
    return ratios, n


def affine_matrix(angles_rad, zoom):
    """R0(a0) . R1(a1) . R2(a2) / zoom in float64: Rk is the right-handed rotation about tensor axis k of (D, H, W), zoom > 1
    magnifies.  The gather reads the volume at patch centre + M (patch index - (roi - 1) / 2)."""
    a0, a1, a2 = (float(a) for a in angles_rad)
    c0, s0, c1, s1, c2, s2 = np.cos(a0), np.sin(a0), np.cos(a1), np.sin(a1), np.cos(a2), np.sin(a2)
    r0 = np.array([[1.0, 0.0, 0.0], [0.0, c0, -s0], [0.0, s0, c0]], dtype=np.float64)
    r1 = np.array([[c1, 0.0, s1], [0.0, 1.0, 0.0], [-s1, 0.0, c1]], dtype=np.float64)
    r2 = np.array([[c2, -s2, 0.0], [s2, c2, 0.0], [0.0, 0.0, 1.0]], dtype=np.float64)
    return (r0 @ r1 @ r2) / float(zoom) + 0.0                  # + 0.0: no negative zeros (zero angles, zoom 1 give eye(3))


def affine_config(prob, rotate, zoom):
    """--t_affine_prob / --t_affine_rotate / --t_affine_zoom as (probability, three angle bounds in degrees, (lo, hi));
    a ValueError names the flag"""
    prob = float(prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"--t_affine_prob takes a probability in [0, 1], got {prob!r}")
    rot = tuple(rotate) if isinstance(rotate, (tuple, list)) else (rotate,)
    if len(rot) == 1:
        rot = rot * 3
    if len(rot) != 3 or any(not float(a) >= 0.0 for a in rot):
        raise ValueError(f"--t_affine_rotate takes one or three angles >= 0 in degrees, got {rotate!r}")
    zm = tuple(zoom) if isinstance(zoom, (tuple, list)) else (zoom,)
    if len(zm) != 2 or not 0.0 < float(zm[0]) <= float(zm[1]):
        raise ValueError(f"--t_affine_zoom takes LO HI with 0 < LO <= HI, got {zoom!r}")
    return prob, tuple(float(a) for a in rot), (float(zm[0]), float(zm[1]))


def draw_affine(rng: np.random.Generator, n, affine):
    """the matrices of n patches, float64 [n, 3, 3]; affine = affine_config(...).  Per patch one uniform number and, only if
    the patch is chosen, three angles and the zoom; a patch not chosen gets the identity.  Probability 0 draws nothing."""
    prob, rot, (lo, hi) = affine
    mats = np.tile(np.eye(3, dtype=np.float64), (n, 1, 1))
    if prob <= 0.0:
        return mats
    for j in range(n):
        if rng.random() < prob:
            ang = [np.deg2rad(float(rng.uniform(-a, a))) for a in rot]
            mats[j] = affine_matrix(ang, float(rng.uniform(lo, hi)))
    return mats


class IntensityRow(C.Structure):
    """mirror of msseg_intensity_row (include/msseg.h): one per (patch, channel)"""
    _fields_ = [("mask", C.c_uint32), ("noise_std", C.c_float), ("noise_key", C.c_uint64), ("blur_sigma", C.c_float),
                ("contrast", C.c_float), ("gamma_inv", C.c_float), ("gamma", C.c_float)]


INTENSITY_STAGES = ("noise", "blur", "contrast", "gamma_invert", "gamma")


def _prob(flag, p):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"--{flag} takes a probability in [0, 1], got {p!r}")
    return p


def _range(flag, v, lowest, open_low, highest=None):
    """LO HI with lowest <(=) LO <= HI (<= highest)"""
    r = tuple(v) if isinstance(v, (tuple, list)) else (v,)
    ok = len(r) == 2 and all(np.isfinite(float(a)) for a in r) and float(r[0]) <= float(r[1]) and \
        (float(r[0]) > lowest if open_low else float(r[0]) >= lowest) and (highest is None or float(r[1]) <= highest)
    if not ok:
        raise ValueError(f"--{flag} takes LO HI with {lowest:g} {'<' if open_low else '<='} LO <= HI"
                         f"{'' if highest is None else f' <= {highest:g}'}, got {v!r}")
    return float(r[0]), float(r[1])


def intensity_config(noise_prob=0.0, noise_std=(0.0, 0.1), blur_prob=0.0, blur_sigma=(0.5, 1.0), blur_channel_prob=0.5,
                     contrast_prob=0.0, contrast_range=(0.75, 1.25), gamma_invert_prob=0.0, gamma_prob=0.0,
                     gamma_range=(0.7, 1.5)):
    """--t_noise_* / --t_blur_* / --t_contrast_* / --t_gamma_* as a dict; a ValueError names the flag.  The blur's HI is
    at most 2: the kernel's radius int(4 sigma + 0.5) stops at 8."""
    return {"noise_prob": _prob("t_noise_prob", noise_prob), "noise_std": _range("t_noise_std", noise_std, 0.0, False),
            "blur_prob": _prob("t_blur_prob", blur_prob), "blur_sigma": _range("t_blur_sigma", blur_sigma, 0.0, True, 2.0),
            "blur_channel_prob": _prob("t_blur_channel_prob", blur_channel_prob),
            "contrast_prob": _prob("t_contrast_prob", contrast_prob),
            "contrast_range": _range("t_contrast_range", contrast_range, 0.0, True),
            "gamma_invert_prob": _prob("t_gamma_invert_prob", gamma_invert_prob),
            "gamma_prob": _prob("t_gamma_prob", gamma_prob), "gamma_range": _range("t_gamma_range", gamma_range, 0.0, True)}


def intensity_config_from_args(cfg):
    """the flags of a parsed command line -> intensity_config(...)"""
    return intensity_config(cfg.t_noise_prob, cfg.t_noise_std, cfg.t_blur_prob, cfg.t_blur_sigma, cfg.t_blur_channel_prob,
                            cfg.t_contrast_prob, cfg.t_contrast_range, cfg.t_gamma_invert_prob, cfg.t_gamma_prob,
                            cfg.t_gamma_range)


def intensity_on(config):
    return config is not None and any(config[s + "_prob"] > 0.0 for s in INTENSITY_STAGES)


def _two_sided(rng, lo, hi):
    """nnU-Net's rule for a factor range that straddles 1: a coin, then U(lo, 1) (only when lo < 1) or U(max(lo, 1), hi);
    the ends are kept inside [lo, hi] when the range lies on one side of 1"""
    if rng.random() < 0.5 and lo < 1.0:
        return float(rng.uniform(lo, min(1.0, hi)))
    return float(rng.uniform(min(max(lo, 1.0), hi), hi))


def draw_intensity(rng: np.random.Generator, n_patches, n_channels, config):
    """the IntensityRow list of n_patches x n_channels (row n * C + c).  Per patch, in the kernel's stage order, one uniform
    number against the stage's probability and, only if the patch is chosen: noise -- one std for the patch, one 64-bit key
    per channel; blur -- per channel one uniform number against blur_channel_prob and, if it passes, a sigma; contrast,
    gamma on the inverted image, gamma -- per channel a factor by _two_sided.  A stage of probability 0 draws nothing; with
    every probability 0 the generator is not touched."""
    rows = [IntensityRow(0, 0.0, 0, 0.0, 1.0, 1.0, 1.0) for _ in range(n_patches * n_channels)]
    if not intensity_on(config):
        return rows
    for j in range(n_patches):
        mine = rows[j * n_channels:(j + 1) * n_channels]
        if config["noise_prob"] > 0.0 and rng.random() < config["noise_prob"]:
            std = float(rng.uniform(*config["noise_std"]))
            for r in mine:
                r.mask |= hip.INTENSITY_NOISE
                r.noise_std, r.noise_key = std, int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        if config["blur_prob"] > 0.0 and rng.random() < config["blur_prob"]:
            for r in mine:
                if rng.random() < config["blur_channel_prob"]:
                    r.mask |= hip.INTENSITY_BLUR
                    r.blur_sigma = float(rng.uniform(*config["blur_sigma"]))
        for stage, bit, field, rng_key in (("contrast", hip.INTENSITY_CONTRAST, "contrast", "contrast_range"),
                                           ("gamma_invert", hip.INTENSITY_GAMMA_INV, "gamma_inv", "gamma_range"),
                                           ("gamma", hip.INTENSITY_GAMMA, "gamma", "gamma_range")):
            if config[stage + "_prob"] > 0.0 and rng.random() < config[stage + "_prob"]:
                for r in mine:
                    r.mask |= bit
                    setattr(r, field, _two_sided(rng, *config[rng_key]))
    return rows


def _check_intensity(config, roi):
    config = intensity_config() if config is None else config
    if intensity_on(config) and roi < 8:
        raise ValueError(f"the intensity augmentation needs patches of at least 8^3, --vol_size is {roi}")
    return config


class DevicePatchLoader:
    """len() batches of `batch` patches of roi^3 from ONE cached volume; deterministic per seed.  affine_prob > 0 sends the
    batch through msseg_aug_crop_affine (see DeviceDatasetLoader); the matrices follow the batch's other draws.  intensity:
    an intensity_config(...) (see DeviceDatasetLoader); the batch's intensity rows follow its matrices."""

    def __init__(self, image: torch.Tensor, label: torch.Tensor, roi: int, batch: int, n_batches: int, device, seed=13,
                 pos=1.0, neg=1.0, flip_prob=0.0, rot_prob=0.0, shift_os=0.1, shift_prob=0.0, scale_f=0.1, scale_prob=0.0,
                 image_threshold=0.0, out_dtype=torch.float32, affine_prob=0.0, affine_rotate=30.0, affine_zoom=(0.7, 1.4),
                 affine_pad=0.0, intensity=None):
        if image.dim() != 4 or label.dim() != 3:
            raise ValueError("image [C, D, H, W] and label [D, H, W] expected")
        self.affine, self.affine_pad = affine_config(affine_prob, affine_rotate, affine_zoom), float(affine_pad)
        self.intensity = _check_intensity(intensity, int(roi))
        self.last_intensity = None
        self.img = image.to(device=device, dtype=torch.float32).contiguous()
        self.lab = label.to(device=device, dtype=torch.uint8).contiguous()
        self.roi, self.batch, self.n, self.dev, self.out_dtype = int(roi), int(batch), int(n_batches), device, out_dtype
        self.cfg = dict(pos=pos, neg=neg, flip_prob=flip_prob, rot_prob=rot_prob, shift_os=shift_os, shift_prob=shift_prob,
                        scale_f=scale_f, scale_prob=scale_prob)
        self.rng = np.random.default_rng(seed)
        # voxel lists of the crop-centre candidates (once per cached volume; index work, stays on the device)
        flat_lab = self.lab.reshape(-1)
        self.fg = torch.nonzero(flat_lab > 0).reshape(-1)
        self.bg = torch.nonzero((flat_lab == 0) & (self.img[0].reshape(-1) > image_threshold)).reshape(-1)
        self.last_rows = self.last_picks = self.last_mats = None
        self.launches = 0
        # the affine gather addresses volumes through a descriptor table: this loader's has one entry
        self.desc = _upload([VolumeDesc(self.img.data_ptr(), self.lab.data_ptr(), *self.img.shape)], device) \
            if self.affine[0] > 0.0 else None

    def __len__(self):
        return self.n

    def rows_for(self, draws):
        """draws -> AugRow list (+ the corrected centres); the centre lookup is one tiny gather from the voxel lists"""
        D, H, W = self.lab.shape
        sel = torch.stack([(self.fg if d[0] else self.bg)[d[1]] for d in draws]).cpu().tolist()
        rows, centers = [], []
        for flat, (use_fg, idx, flips, rotk, shift, scale) in zip(sel, draws):
            c = (flat // (H * W), (flat // W) % H, flat % W)
            c = correct_crop_center(c, (self.roi,) * 3, (D, H, W))
            z0, y0, x0 = (v - self.roi // 2 for v in c)
            rows.append(AugRow(z0, y0, x0, int(flips[0]) | int(flips[1]) << 1 | int(flips[2]) << 2, rotk, 0, shift, scale))
            centers.append(c)
        return rows, centers

    def __iter__(self):
        D, H, W = self.lab.shape
        Cc = self.img.shape[0]
        for _ in range(self.n):
            draws = draw_rows(self.rng, self.batch, int(self.fg.numel()), int(self.bg.numel()), self.cfg)
            rows, centers = self.rows_for(draws)
            self.last_rows = rows
            aug = intensity_on(self.intensity)                   # then the gather writes an fp32 scratch batch
            out = torch.empty(self.batch, Cc, self.roi, self.roi, self.roi, dtype=self.out_dtype, device=self.dev)
            img = torch.empty_like(out, dtype=torch.float32) if aug else out
            lab = torch.empty(self.batch, 1, self.roi, self.roi, self.roi, dtype=torch.float32, device=self.dev)
            if self.affine[0] > 0.0:
                # the matrices are drawn after the batch's other draws; the rows and starts go to the multi-volume gather's
                # tables (one volume, explicit crop starts)
                mats = draw_affine(self.rng, self.batch, self.affine)
                picks = torch.tensor([[c[0], c[1], c[2], r.z0, r.y0, r.x0, 0, 0] for r, c in zip(rows, centers)], dtype=torch.int32)
                table = _upload([PickRow(0, PICK_VOXEL, 0, 0, r.flips, r.rotk, r.shift, r.scale) for r in rows], self.dev)
                hip.aug_crop_affine(self.desc, 1, table, picks.to(self.dev), torch.from_numpy(mats).to(self.dev), img, lab,
                                    self.roi, self.affine_pad)
                self.last_picks, self.last_mats = picks, mats
            else:
                host = torch.frombuffer(bytearray(bytes((AugRow * len(rows))(*rows))), dtype=torch.uint8)
                table = host.to(self.dev, non_blocking=True)
                hip.aug_crop_batch(self.img, self.lab, table, img, lab, self.roi)
            self.launches += 1
            if aug:
                self.last_intensity = draw_intensity(self.rng, self.batch, Cc, self.intensity)
                img = hip.intensity_aug(img, self.last_intensity, self.out_dtype, out=out)
            aff = torch.eye(4)[None].repeat(self.batch, 1, 1)
            cen = torch.tensor(centers, dtype=torch.float32)
            yield {"image": img, "label": lab,
                   "image_meta_dict": {"original_affine": aff, "affine": aff.clone(),
                                       "filename_or_obj": [f"device_cache_{j}" for j in range(self.batch)]},
                   "label_meta_dict": {"affine": aff.clone()},
                   "image_transforms": [{"class": ["RandCropByPosNegLabeld"] * self.batch,
                                         "orig_size": [torch.full((self.batch,), float(s)) for s in (D, H, W)],
                                         "extra_info": {"center": [cen[:, 0], cen[:, 1], cen[:, 2]]}}]}


# ---------------------------------------------------------------------------------------------------------------------
# Dataset path: many preprocessed volumes cached in HBM, batches drawn across them with one gather launch.
# The transforms are the chain of the reference's data/dataset_builder.py:19-217 (training) and :220-306 (validation) up
# to the random crop; MONAI is absent, so what is pinned is parity with the numpy / scipy restatement in
# tests/dataprep_ref.py (MONAI parity unpinned).  Cache cost: 4 bytes per voxel and channel (fp32 image) + 1 (uint8 label)
# + 8 bytes per z-slice of candidate counts; no per-voxel index lists.  The class-ratio crop with a centre dilation adds a
# candidate mask of 2 bytes per voxel per volume for as long as its loader lives (and 1 byte per voxel of scratch while the
# mask is built).
# ---------------------------------------------------------------------------------------------------------------------
class PickRow(C.Structure):
    """mirror of msseg_pick_row (include/msseg.h)"""
    _fields_ = [("vol", C.c_int32), ("mode", C.c_int32), ("z", C.c_int32), ("rank", C.c_int32), ("flips", C.c_int32),
                ("rotk", C.c_int32), ("shift", C.c_float), ("scale", C.c_float)]


class VolumeDesc(C.Structure):
    """mirror of msseg_volume_desc (include/msseg.h)"""
    _fields_ = [("img", C.c_uint64), ("lab", C.c_uint64), ("C", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


PICK_BG, PICK_FG, PICK_VOXEL = 0, 1, 2
# the transform name a batch records for its crop (engine/train.py reads the crop location of any of them)
CROP_TRANSFORM = {"fgbg": "RandCropByPosNegLabeld", "spatial": "RandSpatialCropd", "class_ratios": "RandCropByClassesd"}


def _upload(structs, dev):
    arr = (type(structs[0]) * len(structs))(*structs)
    # a blocking copy: the temporary host buffer is gone when this returns
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def check_transform_flags(cfg):
    """the transform flags this build does not implement raise with the flag's name"""
    hint = {"t_percentile_ct_intensity": " (per-volume percentile clipping: --t_zscore --t_zscore_clip LO HI)",
            "t_normalize_channel_wise": " (per-volume, per-channel normalisation: --t_zscore)",
            "t_rand_crop_classes": " (crop centres per class: --t_rand_crop_class_ratios NEG POS POS ..., one ratio per "
                                   "class, is the same sampler)",
            "t_rand_crop_dilated_center": " (crop centres near a class: --t_rand_crop_class_ratios R0 R1 ... with "
                                          "--t_rand_crop_center_dilation 48)",
            "t_convert_labels_to_brats": " (overlapping label regions with sigmoid outputs: --label_regions SET=VALUE ..., "
                                         "e.g. --output_dim 3 --label_regions 1,2,3=1 2,3=2 3=3; MONAI's mapping changed "
                                         "between releases, so none is built in)"}
    for flag in ("t_percentile_ct_intensity", "t_normalize_channel_wise", "t_crop_foreground_kdiv", "t_rand_crop_classes",
                 "t_rand_crop_dilated_center", "t_convert_labels_to_brats"):
        if getattr(cfg, flag, False) and not (flag == "t_normalize_channel_wise" and not cfg.t_normalize):
            raise NotImplementedError(f"--{flag} is not implemented on the device data path{hint.get(flag, '')}")
    zscore_config(cfg)
    class_crop_config_from_args(cfg)
    region_table(cfg)


def zscore_config(cfg):
    """--t_zscore / --t_zscore_clip -> None (off), () (z-score without clip) or (LO, HI) percentages; a ValueError names
    the flag.  --t_zscore excludes --t_normalize: the cache's pad value, the out-of-volume value of the affine gather and
    the sliding window's cval are the normalised zero, which must stay 0 for the non-zero mask to survive."""
    on = bool(getattr(cfg, "t_zscore", False))
    clip = getattr(cfg, "t_zscore_clip", ())
    clip = tuple(clip) if isinstance(clip, (tuple, list)) else (clip,)
    if clip and not on:
        raise ValueError("--t_zscore_clip needs --t_zscore")
    if not on:
        return None
    if getattr(cfg, "t_normalize", False):
        raise ValueError("--t_zscore and --t_normalize exclude each other: --t_normalize moves the pad value away from 0, "
                         "--t_zscore keeps zeros zero")
    if not clip:
        return ()
    if len(clip) != 2 or not all(np.isfinite(float(q)) for q in clip) or not 0.0 <= float(clip[0]) < float(clip[1]) <= 100.0:
        raise ValueError(f"--t_zscore_clip takes two percentages LO HI with 0 <= LO < HI <= 100, got {clip!r}")
    return float(clip[0]), float(clip[1])


def normalised_zero(cfg):
    """what a scaled intensity of 0 becomes under --t_normalize, in fp32 as the kernel computes it (0.0 without the flag):
    the pad value of the cache and the image threshold of the background crop centres.  The reference thresholds the
    un-normalised image at 0 (RandCropByPosNegLabeld(image_threshold=0) runs in front of NormalizeIntensityd); on the
    normalised cache `v > 0` is `(v - mean) / std > (0 - mean) / std`."""
    if not cfg.t_normalize:
        return 0.0
    return float((np.float32(0.0) - np.float32(cfg.t_norm_mean)) / np.float32(cfg.t_norm_std))


def voxel_dims(cfg):
    """--t_voxel_dims as three spacings: one value is used for every axis"""
    v = cfg.t_voxel_dims
    v = tuple(v) if isinstance(v, (tuple, list)) else (v,)
    if len(v) == 1:
        v = v * 3
    if len(v) != 3 or any(not float(x) > 0 for x in v):
        raise ValueError(f"--t_voxel_dims takes one or three positive spacings, got {cfg.t_voxel_dims!r}")
    return tuple(float(x) for x in v)


def preprocess_volume(image, label, affine, cfg, device, filename="volume"):
    """One loaded case -> the cached record.  image: numpy [C, X, Y, Z] (int16 / float32 / other numeric), label numpy
    [X, Y, Z] or None.  Chain: Orientationd(RAS) when in_chans == 1 -> Spacingd -> intensity scaling (+ NormalizeIntensityd)
    with the foreground box -> CropForegroundd -> SpatialPadd(vol_size).  NormalizeIntensityd is applied here for training
    as well: the reference applies it after the random shift / scale, this cache before them (the pad value is the
    normalised zero, as a pad before the normalisation gives; the background crop centres must then be thresholded at
    normalised_zero(cfg), not at 0).  With --t_zscore the chain ends with the per-volume z-score of every channel over its
    non-zero voxels (hip.zscore_nonzero_; zeros and pads stay 0, the background crop centres are then the voxels != 0:
    DeviceDatasetLoader(image_rule="ne")); the record's "zscore" is the host copy of the statistics, float64 [C, 6] =
    {n, P_LO, P_HI, mean, std, non-finite count}."""
    from . import data_files as df
    check_transform_flags(cfg)
    zscore = zscore_config(cfg)
    roi = cfg.vol_size if isinstance(cfg.vol_size, int) else cfg.vol_size[0]
    image = np.asarray(image)
    if image.dtype != np.int16 and image.dtype != np.float32:
        image = image.astype(np.float32)
    img = torch.from_numpy(np.ascontiguousarray(image)).to(device)
    lab = torch.from_numpy(np.ascontiguousarray(label).astype(np.uint8)).to(device) if label is not None else \
        torch.zeros(image.shape[1:], dtype=torch.uint8, device=device)
    original_affine = np.array(affine, dtype=np.float64)
    aff = original_affine.copy()
    native_shape = tuple(int(s) for s in image.shape[1:])
    perm, flips, spacing_scale = (0, 1, 2), (False, False, False), (1.0, 1.0, 1.0)
    if cfg.in_chans == 1:
        perm, flips = df.ras_orientation(aff)
        aff = df.reorient_affine(aff, tuple(img.shape[1:]), perm, flips)
        img = img.permute(0, *(1 + p for p in perm))
        lab = lab.permute(*perm)
        fl = [a for a in range(3) if flips[a]]
        if fl:
            img, lab = img.flip([1 + a for a in fl]), lab.flip(fl)
        img, lab = img.contiguous(), lab.contiguous()
    if cfg.t_voxel_spacings:
        new = voxel_dims(cfg)
        old = df.spacing_of(aff)
        ratio = [float(n) / float(o) for n, o in zip(new, old)]
        spacing_scale = tuple(float(o) / float(n) for n, o in zip(new, old))
        out = [df.resample_shape(s, o, n) for s, o, n in zip(img.shape[1:], old, new)]
        if img.dtype != torch.float32:
            img, _ = hip.intensity_prep(img)                    # int16 -> fp32, values unchanged
        img = hip.resample_spacing(img, out, ratio)
        lab = hip.resample_spacing(lab[None], out, ratio)[0]
        aff = df.rescale_affine(aff, ratio)
    mode = hip.INTENSITY_CUBED if cfg.t_cubed_ct_intensity else hip.INTENSITY_RANGE if cfg.t_fixed_ct_intensity else hip.INTENSITY_NONE
    norm = (cfg.t_norm_mean, cfg.t_norm_std) if cfg.t_normalize else None
    img, box = hip.intensity_prep(img, mode, cfg.t_ct_min, cfg.t_ct_max, norm)
    pad = normalised_zero(cfg)
    D, H, W = img.shape[1:]
    grid_shape = (int(D), int(H), int(W))
    b6 = (0, 0, 0, D, H, W)
    if cfg.t_crop_foreground_img:
        b = box.cpu().tolist()
        if b[3] >= 0:                                            # an empty foreground keeps the whole volume
            b6 = (b[0], b[1], b[2], b[3] + 1, b[4] + 1, b[5] + 1)
    min_size = (roi,) * 3 if cfg.t_spatial_pad else None
    before = (0, 0, 0)
    if b6 != (0, 0, 0, D, H, W) or (min_size and min(D, H, W) < roi):
        img, before = hip.crop_pad_copy(img, b6, min_size, pad)
        lab = hip.crop_pad_copy(lab[None], b6, min_size, 0)[0][0]
        aff = df.shift_affine(aff, [b6[a] - before[a] for a in range(3)])
    extra = {}
    if zscore is not None:
        # last: the pads (0) and every other zero stay outside the statistics and stay zero
        img = img.contiguous()
        stats = hip.zscore_nonzero_(img, zscore or None).cpu().numpy()     # the one small read-back: [C, 6]
        if not np.isfinite(stats[:, 3:5]).all() or stats[:, 5].any():
            raise ValueError(f"{filename}: --t_zscore met a NaN or an infinite intensity (per channel: "
                             f"{[int(v) for v in stats[:, 5]]} non-finite voxel(s), mean {stats[:, 3].tolist()}, "
                             f"std {stats[:, 4].tolist()})")
        extra["zscore"] = stats
    return {**extra, "img": img,"lab": lab.contiguous(), "affine": aff, "original_affine": original_affine, "filename": filename,
            "box": b6, "pad_before": tuple(before),
            # the geometry restore_descriptor needs to map a prediction back onto the file's grid
            "native_shape": native_shape, "orient": (tuple(int(p) for p in perm), tuple(bool(f) for f in flips)),
            "spacing_scale": spacing_scale, "grid_shape": grid_shape, "model_shape": tuple(int(s) for s in lab.shape)}


RESTORE_KEYS = ("native_shape", "orient", "spacing_scale", "grid_shape", "box", "pad_before", "model_shape")


def restore_geometry(rec):
    """the keys of a preprocess_volume record that restore_descriptor reads, without the tensors: what a batch carries as
    its "restore" entry (with the file's affine in float64, which the native map is saved under)"""
    return {**{k: rec[k] for k in RESTORE_KEYS}, "original_affine": np.array(rec["original_affine"], dtype=np.float64)}


def restore_descriptor(rec):
    """A preprocess_volume record, or any dict with its keys native_shape, orient, spacing_scale, grid_shape, box,
    pad_before and model_shape (or lab, whose shape is then the model grid) -> hip.RestoreDesc, the msseg_restore_desc of
    include/msseg.h: the inverse of the record's chain.  Pure host code."""
    perm, flips = rec["orient"]
    model = rec["model_shape"] if "model_shape" in rec else tuple(rec["lab"].shape)
    d = hip.RestoreDesc()
    for k in range(3):
        d.native[k], d.perm[k], d.flip[k] = int(rec["native_shape"][k]), int(perm[k]), int(bool(flips[k]))
        d.grid[k], d.model[k] = int(rec["grid_shape"][k]), int(model[k])
        d.offset[k] = int(rec["pad_before"][k]) - int(rec["box"][k])
        d.scale[k] = float(rec["spacing_scale"][k])
    return d


def build_cache(files, cfg, device):
    """read, preprocess and keep every case of `files` on the device -> (records, cached bytes)"""
    from . import data_files as df
    recs, nbytes = [], 0
    for item in files:
        image, label, aff = df.load_case(item)
        if image.shape[0] != cfg.in_chans:
            raise ValueError(f"{item['image']}: {image.shape[0]} channel(s), --in_chans is {cfg.in_chans}")
        r = preprocess_volume(image, label, aff, cfg, device, filename=item["image"])
        nbytes += r["img"].numel() * 4 + r["lab"].numel()
        recs.append(r)
    return recs, nbytes


def _aff(recs, key):
    return torch.stack([torch.from_numpy(np.asarray(r[key])).float() for r in recs])


class DeviceDatasetLoader:
    """len() batches of `batch` patches of roi^3 drawn across the cached `volumes` (records of preprocess_volume): a seeded
    permutation of the volumes per epoch, `patches_per_image` consecutive patches from each, the per-patch draws of
    draw_rows; msseg_pick_voxels resolves the crop centres from the per-slice candidate counts and msseg_aug_crop_multi
    writes the batch in ONE launch.  crop = "fgbg" (RandCropByPosNegLabeld) or "spatial" (RandSpatialCropd).
    affine_prob > 0: each patch is, with that probability, rotated (angles from U(-affine_rotate, affine_rotate) degrees per
    tensor axis) and zoomed (factor from U(*affine_zoom)) about its centre by sampling the cached volume under
    affine_matrix(...) in msseg_aug_crop_affine, still one launch; taps outside the volume read affine_pad.  The matrices
    of the last batch are in last_mats.  With affine_prob == 0 nothing changes: same kernels, same generator stream.
    intensity: an intensity_config(...).  With any of its stages on, the gather writes an fp32 scratch batch, a patch's
    intensity rows (draw_intensity) are drawn after its other draws and its matrix, and msseg_intensity_aug (noise, blur,
    contrast, gamma inverted, gamma) writes the batch in out_dtype; the rows of the last batch are in last_intensity, the
    labels are untouched.  With every stage off: no draw, no scratch, no launch.
    image_rule: the image side of a background crop centre, "gt" = image[0] > image_threshold, "ne" = image[0] !=
    image_threshold: for a z-scored cache (--t_zscore), where the reference's `raw image > 0` is the non-zero mask and the
    in-mask values have either sign (a voxel whose z-score is exactly 0.0 drops out of the candidates).
    crop = "class_ratios" (RandCropByLabelClassesd) with class_ratios = one ratio >= 0 per class (K <= 16) and
    center_dilation = N in 0..254: voxel v is a candidate of class c iff the image rule holds at v (for every class,
    channel 0) and a voxel of label c lies within L1 distance N of v (N = 0: v itself has label c); labels >= K belong to
    no class.  Per patch draw_class_rows picks the class (ratios of the classes the volume has no candidate of zeroed, the
    rest renormalised) and the candidate; msseg_class_pick_voxels resolves it from the per-slice, per-class counts.  With
    N > 0 every cached volume gets a uint16 candidate mask at construction (msseg_class_candidate_mask, for the classes
    of positive ratio; 2 bytes per voxel for as long as the loader lives).  class_candidates[volume][class] are the totals,
    last_classes the class of each patch of the last batch (-1: no candidate at all, a uniform voxel).  With class_ratios
    and center_dilation at their defaults nothing changes for "fgbg" and "spatial": same kernels, same generator stream, no
    extra memory."""

    def __init__(self, volumes, roi, batch, n_batches, patches_per_image=1, device=None, seed=13, crop="fgbg", pos=1.0,
                 neg=1.0, flip_prob=0.0, rot_prob=0.0, shift_os=0.1, shift_prob=0.0, scale_f=0.1, scale_prob=0.0,
                 image_threshold=0.0, out_dtype=torch.float32, affine_prob=0.0, affine_rotate=30.0, affine_zoom=(0.7, 1.4),
                 affine_pad=0.0, intensity=None, image_rule="gt", class_ratios=None, center_dilation=0):
        self.affine, self.affine_pad = affine_config(affine_prob, affine_rotate, affine_zoom), float(affine_pad)
        self.intensity = _check_intensity(intensity, int(roi))
        self.last_intensity = None
        if image_rule not in hip.BG_RULES:
            raise ValueError(f"image_rule {image_rule!r}: 'gt' or 'ne'")
        self.image_rule = image_rule
        if not volumes:
            raise ValueError("DeviceDatasetLoader needs at least one cached volume")
        if crop not in ("fgbg", "spatial", "class_ratios"):
            raise NotImplementedError(f"crop mode {crop!r}: --t_rand_crop_fgbg, --t_rand_spatial_crop and "
                                      f"--t_rand_crop_class_ratios (\"class_ratios\") are implemented")
        self.class_ratios, self.center_dilation = class_crop_config(class_ratios, center_dilation)
        if (self.class_ratios is not None) != (crop == "class_ratios"):
            raise ValueError("crop=\"class_ratios\" and class_ratios (--t_rand_crop_class_ratios) go together")
        self.vols, self.roi, self.batch, self.n = list(volumes), int(roi), int(batch), int(n_batches)
        self.ppi, self.dev, self.crop, self.thr, self.out_dtype = max(int(patches_per_image), 1), device, crop, float(image_threshold), out_dtype
        self.cfg = dict(pos=pos, neg=neg, flip_prob=flip_prob, rot_prob=rot_prob, shift_os=shift_os, shift_prob=shift_prob,
                        scale_f=scale_f, scale_prob=scale_prob)
        self.rng = np.random.default_rng(seed)
        self.C = int(self.vols[0]["img"].shape[0])
        descs = []
        for v in self.vols:
            img, lab = v["img"], v["lab"]
            if img.dtype != torch.float32 or lab.dtype != torch.uint8 or not img.is_cuda or not lab.is_cuda or \
                    not img.is_contiguous() or not lab.is_contiguous() or img.dim() != 4 or tuple(img.shape[1:]) != tuple(lab.shape):
                raise ValueError("cached volumes: contiguous fp32 [C, D, H, W] image and uint8 [D, H, W] label on the GPU")
            if img.shape[0] != self.C or min(img.shape[1:]) < self.roi:
                raise ValueError(f"{v['filename']}: volume {tuple(img.shape)} does not hold a {self.roi}^3 patch of {self.C} "
                                 f"channel(s) (--t_spatial_pad pads small volumes)")
            descs.append(VolumeDesc(img.data_ptr(), lab.data_ptr(), *img.shape))
        self.desc = _upload(descs, device)
        # candidate counts per z-slice, cumulative on the host: 8 bytes per slice instead of 8 bytes per voxel
        self.cum = []
        if crop == "fgbg":
            counts = [hip.slab_counts(v["img"], v["lab"], self.thr, self.image_rule) for v in self.vols]
            for c in counts:
                c = c.cpu().numpy().astype(np.int64)
                self.cum.append((np.cumsum(c[:, 0]), np.cumsum(c[:, 1])))
        # class-ratio crop: [D, K] cumulative counts per volume; with a dilation the candidate masks (2 bytes per voxel)
        self.class_cum, self.class_candidates, self.masks, self.mask_ptrs = [], [], [], None
        self.last_classes = None
        if crop == "class_ratios":
            K = len(self.class_ratios)
            if self.center_dilation > 0:
                live = [c for c in range(K) if self.class_ratios[c] > 0.0]
                self.masks = [hip.class_candidate_mask(v["img"], v["lab"], live, self.center_dilation, self.thr, self.image_rule)
                              for v in self.vols]
                self.mask_ptrs = torch.tensor([m.data_ptr() for m in self.masks], dtype=torch.int64).to(device)
            counts = [hip.class_slab_counts(v["img"], v["lab"], K, self.thr, self.image_rule,
                                            mask=self.masks[k] if self.masks else None) for k, v in enumerate(self.vols)]
            for c in counts:
                self.class_cum.append(np.cumsum(c.cpu().numpy().astype(np.int64), axis=0))
                self.class_candidates.append([int(t) for t in self.class_cum[-1][-1]])
        self.order, self.taken = [], 0
        self.launches = 0
        self.last_rows = self.last_picks = self.last_mats = None

    def __len__(self):
        return self.n

    def _next_volume(self):
        """volume of the next patch: a new seeded permutation whenever the last one is used up"""
        if self.taken == 0:
            if not self.order:
                self.order = list(self.rng.permutation(len(self.vols)))
            self.current = int(self.order.pop(0))
        self.taken = (self.taken + 1) % self.ppi
        return self.current

    def _row(self, vi):
        D, H, W = self.vols[vi]["lab"].shape
        if self.crop == "spatial":
            (_, _, flips, rotk, shift, scale), = draw_rows(self.rng, 1, 0, 1, self.cfg)
            start = [int(self.rng.integers(0, n - self.roi + 1)) for n in (D, H, W)]
            fl = int(flips[0]) | int(flips[1]) << 1 | int(flips[2]) << 2
            return PickRow(vi, PICK_VOXEL, 0, 0, fl, rotk, shift, scale), start
        if self.crop == "class_ratios":
            (cls, idx, flips, rotk, shift, scale), = draw_class_rows(self.rng, 1, self.class_candidates[vi], self.class_ratios,
                                                                     self.cfg)
            fl = int(flips[0]) | int(flips[1]) << 1 | int(flips[2]) << 2
            self._classes.append(cls)
            if cls < 0:                                              # no candidate at all: a uniform voxel of the volume
                flat = int(self.rng.integers(0, D * H * W))
                return PickRow(vi, PICK_VOXEL, flat // (H * W), flat % (H * W), fl, rotk, shift, scale), None
            cum = self.class_cum[vi][:, cls]
            z = int(np.searchsorted(cum, idx, side="right"))
            rank = idx - (int(cum[z - 1]) if z else 0)
            return PickRow(vi, hip.PICK_CLASS0 + cls, z, rank, fl, rotk, shift, scale), None
        cf, cb = self.cum[vi]
        nf, nb = int(cf[-1]), int(cb[-1])
        (use_fg, idx, flips, rotk, shift, scale), = draw_rows(self.rng, 1, nf, nb, self.cfg)
        fl = int(flips[0]) | int(flips[1]) << 1 | int(flips[2]) << 2
        if nf == 0 and nb == 0:                                  # no candidate at all: a uniform voxel of the volume
            flat = int(self.rng.integers(0, D * H * W))
            return PickRow(vi, PICK_VOXEL, flat // (H * W), flat % (H * W), fl, rotk, shift, scale), None
        cum = cf if use_fg else cb
        z = int(np.searchsorted(cum, idx, side="right"))
        rank = idx - (int(cum[z - 1]) if z else 0)
        return PickRow(vi, PICK_FG if use_fg else PICK_BG, z, rank, fl, rotk, shift, scale), None

    def __iter__(self):
        R = self.roi
        for _ in range(self.n):
            vis = [self._next_volume() for _ in range(self.batch)]
            aug = intensity_on(self.intensity)
            # a patch's matrix is drawn right after its other draws, its intensity rows after the matrix
            made, irows, self._classes = [], [], []
            mats = np.empty((self.batch, 3, 3), dtype=np.float64) if self.affine[0] > 0.0 else None
            for j, vi in enumerate(vis):
                made.append(self._row(vi))
                if mats is not None:
                    mats[j] = draw_affine(self.rng, 1, self.affine)[0]
                if aug:
                    irows += draw_intensity(self.rng, 1, self.C, self.intensity)
            rows = [m[0] for m in made]
            table = _upload(rows, self.dev)
            if self.crop == "spatial":
                host = torch.tensor([[s[0] + R // 2, s[1] + R // 2, s[2] + R // 2, s[0], s[1], s[2], 0, 0] for _, s in made],
                                    dtype=torch.int32)
                picks = host.to(self.dev, non_blocking=True)
            else:
                picks = torch.empty(self.batch, 8, dtype=torch.int32, device=self.dev)
                if self.crop == "class_ratios":
                    hip.class_pick_voxels(self.desc, len(self.vols), table, self.batch, R, self.thr, picks, self.image_rule,
                                          masks=self.mask_ptrs)
                else:
                    hip.pick_voxels(self.desc, len(self.vols), table, self.batch, R, self.thr, picks, self.image_rule)
            out = torch.empty(self.batch, self.C, R, R, R, dtype=self.out_dtype, device=self.dev)
            img = torch.empty_like(out, dtype=torch.float32) if aug else out   # the gather's fp32 scratch batch
            lab = torch.empty(self.batch, 1, R, R, R, dtype=torch.float32, device=self.dev)
            if mats is None:
                hip.aug_crop_multi(self.desc, len(self.vols), table, picks, img, lab, R)
            else:
                hip.aug_crop_affine(self.desc, len(self.vols), table, picks, torch.from_numpy(mats).to(self.dev), img, lab, R,
                                    self.affine_pad)
            self.launches += 1
            if aug:
                img = hip.intensity_aug(img, irows, self.out_dtype, out=out)
                self.last_intensity = irows
            if self.crop != "spatial":
                host = picks.cpu()                               # the one small device-to-host copy of the batch
            self.last_rows, self.last_picks, self.last_mats = rows, host, mats
            self.last_classes = list(self._classes) if self.crop == "class_ratios" else None
            cen = host[:, :3].float()
            recs = [self.vols[vi] for vi in vis]
            sizes = [[float(r["lab"].shape[a]) for r in recs] for a in range(3)]
            yield {"image": img, "label": lab,
                   "image_meta_dict": {"original_affine": _aff(recs, "original_affine"), "affine": _aff(recs, "affine"),
                                       "filename_or_obj": [r["filename"] for r in recs]},
                   "label_meta_dict": {"affine": _aff(recs, "affine")},
                   "image_transforms": [{"class": [CROP_TRANSFORM[self.crop]] * self.batch,
                                         "orig_size": [torch.tensor(s) for s in sizes],
                                         "extra_info": {"center": [cen[:, 0], cen[:, 1], cen[:, 2]]}}]}


class DeviceVolumeLoader:
    """validation: one cached, preprocessed whole volume per step (batch 1), in the engine's batch-dict layout"""

    def __init__(self, volumes):
        self.vols = list(volumes)

    def __len__(self):
        return len(self.vols)

    def __iter__(self):
        for r in self.vols:
            yield {"image": r["img"][None], "label": r["lab"][None, None].float(),
                   "image_meta_dict": {"original_affine": _aff([r], "original_affine"), "affine": _aff([r], "affine"),
                                       "filename_or_obj": [r["filename"]]},
                   "label_meta_dict": {"affine": _aff([r], "affine")},
                   "image_transforms": []}


def output_name(path):
    """the name test_model saves a case under: the file's base name behind its last "img" (the reference's rule,
    engine/test.py:127 there)"""
    return os.path.split(str(path))[-1].split("img")[-1]


def check_output_names(files):
    """two cases of one output name would overwrite each other's maps: a ValueError names both files"""
    seen = {}
    for item in files:
        name = output_name(item["image"])
        if name in seen:
            raise ValueError(f"{item['image']} and {seen[name]} would both be saved as {name!r}")
        seen[name] = item["image"]


class FileCaseLoader:
    """test-time inference on files: one case per step (batch 1), read and preprocessed when the step asks for it and not
    kept afterwards (no whole-set cache); labels, if the data list names any, are ignored.  The batch carries the record's
    geometry as "restore", which engine.test.test_model maps the prediction back onto the file's grid with."""

    def __init__(self, files, cfg, device):
        self.files, self.cfg, self.dev = list(files), cfg, device
        check_output_names(self.files)

    def __len__(self):
        return len(self.files)

    def __iter__(self):
        from . import data_files as df
        for item in self.files:
            image, _, aff = df.load_case({"image": item["image"]})
            if image.shape[0] != self.cfg.in_chans:
                raise ValueError(f"{item['image']}: {image.shape[0]} channel(s), --in_chans is {self.cfg.in_chans}")
            r = preprocess_volume(image, None, aff, self.cfg, self.dev, filename=item["image"])
            batch = {"image": r["img"][None],
                     "image_meta_dict": {"original_affine": _aff([r], "original_affine"), "affine": _aff([r], "affine"),
                                         "filename_or_obj": [r["filename"]]},
                     "image_transforms": [], "restore": restore_geometry(r)}
            del r, image
            yield batch
            del batch


def crop_mode(cfg):
    """the crop flag of a command line -> DeviceDatasetLoader's crop mode: "fgbg" (--t_rand_crop_fgbg), "spatial"
    (--t_rand_spatial_crop) or "class_ratios" (--t_rand_crop_class_ratios, whose ratios and dilation
    class_crop_config_from_args returns); two crop flags at once are a ValueError that names both"""
    check_transform_flags(cfg)
    if class_crop_config_from_args(cfg)[0] is not None:
        return "class_ratios"
    if cfg.t_rand_crop_fgbg:
        return "fgbg"
    if cfg.t_rand_spatial_crop:
        return "spatial"
    raise SystemExit("training on files needs a crop flag: --t_rand_crop_fgbg, --t_rand_spatial_crop or "
                     "--t_rand_crop_classes (the last one is not implemented on the device data path), or "
                     "--t_rand_crop_class_ratios R0 R1 ... (crop centres per class, one ratio per class)")


def dataset_file_lists(cfg, rank, world):
    """-> (this rank's training files, this rank's validation files, all training files, all validation files):
    the "validation" section when the data list has one, the cross-validation split otherwise; both partitioned over the
    ranks as dataset_builder.py:455-463 does"""
    from . import data_files as df
    js = df.datalist_path(cfg.data_path, cfg.task, cfg.json_list)
    if df.has_key(js, "validation"):
        train, val = df.load_datalist(js, "training"), df.load_datalist(js, "validation")
    else:
        train, val = df.cv_split(df.load_datalist(js, "training"), cfg.seed, cfg.cv_max_folds, cfg.cv_fold)
    return df.partition(train, world, rank), df.partition(val, world, rank), train, val
