#!/usr/bin/env python
"""Scores a folder of native-grid label maps (``run_predict.py``'s ``native/``, or ``majority_vote.py``'s
``voted_output/native/``) against the label files of a Decathlon data list: per case and class the Dice score and, in
millimetres on the file's own grid, the Hausdorff percentile, the average symmetric surface distance and the normalised
surface Dice (``metrics.surface_metrics``).  A prediction is matched by NAME (``data_device.output_name`` of the case's
image) to a labelled entry of the data list's ``training`` / ``validation`` sections; a name without a labelled partner, a
shape or an affine that differs from the label file's are errors, found for every file before the first one is scored.
Single process, one case on the device at a time.

    python run_score.py --pred_folder out/test_output/Fold0/native --data_path /data --task Task09_Spleen --n_classes 2

With ``--label_regions SET=VALUE ...`` (the flag of the training drivers) the rows are REGIONS, unions of label values, instead
of classes: both maps are taken through each region's label set to {0, 1} and scored as a two-class pair
(``score_regions``); ``--n_classes`` is not needed, ``--nsd_tolerance`` holds one value or one per region, and every region
counts as foreground.

    python run_score.py --pred_folder out/test_output/Fold0/native --data_path /data --task Task01_BrainTumour \\
        --label_regions 1,2,3=1 2,3=2 3=3
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METRICS = ("dice", "hd_mm", "assd_mm", "nsd")
AFFINE_ATOL = 1e-3      # both affines come from one header through save_nifti's float32 sform: a condition, not a measurement


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Dice, HD percentile, ASSD and NSD (mm) of native-grid label maps")
    parser.add_argument("--pred_folder", type=str, required=True,
                        help="e.g. out/test_output/Fold0/native or out/test_output/voted_output/native")
    parser.add_argument("--data_path", type=str, required=True)
    parser.add_argument("--task", type=str, required=True)
    parser.add_argument("--json_list", type=str, default="dataset.json")
    parser.add_argument("--n_classes", type=int, default=None, help="needed unless --label_regions is given")
    parser.add_argument("--label_regions", type=str, nargs="*", default=[],
                        help="score regions (unions of label values) instead of classes: one SET=VALUE token per region as "
                             "in training, e.g. 1,2,3=1 2,3=2 3=3 (the VALUE part is not used here)")
    parser.add_argument("--nsd_tolerance", type=float, nargs="+", default=[1.0],
                        help="surface Dice tolerance in mm: one value, or one per class (background included).  Decathlon's "
                             "tolerances are set per task and organ; 1.0 is only a default")
    parser.add_argument("--percentile", type=float, default=95.0)
    parser.add_argument("--out", type=str, default=None, help="default: <pred_folder>/scores.json")
    return parser


def labelled_cases(json_path):
    """output name -> data-list entry, over the labelled entries of the "training" and "validation" sections"""
    from medicalsemseg_amd import data_device, data_files
    items = []
    for key in ("training", "validation"):
        if data_files.has_key(json_path, key):
            items += [it for it in data_files.load_datalist(json_path, key) if it.get("label")]
    data_device.check_output_names(items)
    return {data_device.output_name(it["image"]): it for it in items}


def match_predictions(pred_folder, json_path):
    """-> [(name, prediction path, label path)] for the NIfTI names of pred_folder, sorted; SystemExit names a prediction
    that no labelled entry of the data list is saved under"""
    if not os.path.isdir(pred_folder):
        raise SystemExit(f"{pred_folder}: no such folder")
    cases = labelled_cases(json_path)
    out = []
    for name in sorted(n for n in os.listdir(pred_folder) if n.endswith((".nii", ".nii.gz"))):
        if name not in cases:
            raise SystemExit(f"{name}: no labelled case of {json_path} is saved under this name")
        out.append((name, os.path.join(pred_folder, name), cases[name]["label"]))
    if not out:
        raise SystemExit(f"{pred_folder}: no NIfTI files")
    return out


def check_pair(name, pred_path, label_path):
    """the prediction must lie on the label file's grid: same shape, same affine (AFFINE_ATOL on every entry); headers only.
    -> the spacing of the three array axes in mm"""
    import numpy as np

    from medicalsemseg_amd import data_files
    from medicalsemseg_amd.utils.nifti import read_nifti_header
    p_shape, p_aff = read_nifti_header(pred_path)
    l_shape, l_aff = read_nifti_header(label_path)
    if p_shape != l_shape:
        raise SystemExit(f"{name}: shape {p_shape}, the label file {label_path} has {l_shape}")
    if len(l_shape) != 3:
        raise SystemExit(f"{name}: {len(l_shape)}-D label map; 3-D expected")
    worst = float(np.abs(p_aff - l_aff).max())
    if not worst <= AFFINE_ATOL:
        raise SystemExit(f"{name}: affine differs from the label file's ({label_path}) by {worst:g} (limit {AFFINE_ATOL:g}): "
                         "the map is on another grid")
    return [float(s) for s in data_files.spacing_of(l_aff)]


def score_regions(pred, label, masks, spacing, nsd_tolerance, percentile=95.0):
    """uint8 maps on the device -> {metric: [R values]} per region of bit mask masks[r]: both maps go through a 256-entry
    table to {0, 1} (a torch index: a cold path) and class 1 of ``metrics.surface_metrics(.., 2, ..)`` is the region's row;
    the Dice comes from ``hip.region_counts_u8``.  nsd_tolerance: one value, or one per region."""
    import numpy as np
    import torch

    from medicalsemseg_amd import hip, metrics
    from medicalsemseg_amd.engine.test import region_lut
    from medicalsemseg_amd.losses import dice_from_counts
    tol = np.broadcast_to(np.asarray(nsd_tolerance, dtype=np.float64).reshape(-1), (len(masks),)) \
        if len(nsd_tolerance) in (1, len(masks)) else None
    if tol is None:
        raise ValueError(f"--nsd_tolerance must hold one value or one per region ({len(masks)})")
    out = {m: [] for m in METRICS}
    counts = hip.region_counts_u8(pred.reshape(-1).contiguous(), label.reshape(-1).contiguous(), masks)
    out["dice"] = dice_from_counts(counts[None])[0][0].double().cpu().tolist()
    for r, mask in enumerate(masks):
        lut = region_lut(mask, pred.device)
        surf = metrics.surface_metrics(lut[pred.long()], lut[label.long()], 2, spacing, [float(tol[r])], percentile)
        for m in ("hd_mm", "assd_mm", "nsd"):
            out[m].append(float(surf[m][1]))
    return out


def summarise(cases, n_classes, regions=False):
    """cases: name -> {metric: [n_classes]} -> {"per_class": [..], "foreground": ..}: the mean of every metric over its finite
    values, the number of cases, and n_missed = the number of non-finite hd_mm (inf: one map lacks the class; NaN: both do).
    regions: the rows are regions -- keyed "region" as well, and all of them foreground"""
    import numpy as np
    vals = {m: np.array([[c[m][k] for k in range(n_classes)] for c in cases.values()], dtype=np.float64).reshape(-1, n_classes)
            for m in METRICS}

    def row(cols):
        r = {}
        for m in METRICS:
            v = vals[m][:, cols].reshape(-1)
            fin = v[np.isfinite(v)]
            r[m] = float(fin.mean()) if fin.size else float("nan")
        r["n_cases"] = len(cases)
        r["n_missed"] = int((~np.isfinite(vals["hd_mm"][:, cols])).sum())
        return r

    if regions:
        return {"per_class": [dict(row([k]), **{"class": k, "region": k}) for k in range(n_classes)],
                "foreground": row(list(range(n_classes)))}
    return {"per_class": [dict(row([k]), **{"class": k}) for k in range(n_classes)],
            "foreground": row(list(range(1, n_classes)))}


def print_table(summary, regions=False):
    print(f"{('region' if regions else 'class'):>10} {'Dice':>8} {'HD (mm)':>9} {'ASSD (mm)':>10} {'NSD':>8} {'cases':>6} {'missed':>7}")
    for label, r in [(str(r["class"]), r) for r in summary["per_class"]] + [("foreground", summary["foreground"])]:
        print(f"{label:>10} {r['dice']:8.4f} {r['hd_mm']:9.3f} {r['assd_mm']:10.3f} {r['nsd']:8.4f} {r['n_cases']:6d} "
              f"{r['n_missed']:7d}")


def main(args):
    from medicalsemseg_amd import data_files
    from medicalsemseg_amd.utils.arguments import parse_label_regions
    tokens = list(getattr(args, "label_regions", None) or [])
    masks = None
    if tokens:
        try:
            masks = parse_label_regions(tokens, len(tokens))[0]
        except ValueError as e:
            raise SystemExit(str(e))
        args.n_classes = len(masks)                              # the number of rows
    if args.n_classes is None or args.n_classes < 1 or len(args.nsd_tolerance) not in (1, args.n_classes):
        raise SystemExit("--n_classes (or --label_regions) is needed, --n_classes must be at least 1 and --nsd_tolerance must "
                         "hold one value or one per class (per region under --label_regions)")
    js = data_files.datalist_path(args.data_path, args.task, args.json_list)
    pairs = match_predictions(args.pred_folder, js)
    spacings = [check_pair(*p) for p in pairs]                   # every refusal comes before the device is touched

    import numpy as np
    import torch

    from medicalsemseg_amd import metrics
    from medicalsemseg_amd.utils.nifti import load_nifti
    if not torch.cuda.is_available():
        raise SystemExit("run_score.py needs an MI355X: medicalsemseg_amd has no CPU fallback")
    cases = {}
    for (name, pred_path, label_path), spacing in zip(pairs, spacings):
        pred = torch.from_numpy(np.ascontiguousarray(load_nifti(pred_path)[0]).astype(np.uint8)).cuda()
        label = torch.from_numpy(np.ascontiguousarray(load_nifti(label_path)[0]).astype(np.uint8)).cuda()
        if masks is not None:
            cases[name] = dict(score_regions(pred, label, masks, spacing, args.nsd_tolerance, args.percentile), spacing=spacing)
            continue
        dice, _ = metrics.dice_from_maps(pred, label, args.n_classes)
        surf = metrics.surface_metrics(pred, label, args.n_classes, spacing, args.nsd_tolerance, args.percentile)
        cases[name] = dict({k: v.tolist() for k, v in surf.items()}, dice=dice[0].double().cpu().tolist(), spacing=spacing)
    summary = summarise(cases, args.n_classes, regions=masks is not None)
    out = args.out or os.path.join(args.pred_folder, "scores.json")
    with open(out, "w") as f:      # NaN / Infinity as Python's json writes and reads them
        json.dump({"pred_folder": os.path.abspath(args.pred_folder), "data_list": js, "n_classes": args.n_classes,
                   "nsd_tolerance": args.nsd_tolerance, "percentile": args.percentile, "cases": cases, "summary": summary,
                   **({"label_regions": tokens} if tokens else {})},
                  f, indent=1)
    print_table(summary, regions=masks is not None)
    print(f"scored {len(cases)} file(s) -> {out}")


if __name__ == "__main__":
    main(build_parser().parse_args())
