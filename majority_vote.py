#!/usr/bin/env python
"""Fold ensembling of saved label maps: the command line of ``/root/reference/majority_vote.py``.  For every file name in
``<in_folder>/Fold0/<prefix>/`` the maps ``Fold<k>/<prefix>/<same name>`` of all folds are voted on the device
(``hip.majority_vote_u8``: one vote per fold for its foreground class, background starts with one vote, first maximum)
and written to ``<in_folder>/voted_output/<prefix>/<name>`` with the first fold's affine.  Files are matched by NAME (the
reference pairs them by their position in a glob); a name that some fold lacks is an error.

    python majority_vote.py --in_folder out/test_output --n_classes 3 --subfolder_prefix native --folds 5
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="majority vote over the label maps of several folds")
    parser.add_argument("--in_folder", type=str, required=True, help="the folder that holds Fold0 .. Fold<folds - 1>")
    parser.add_argument("--n_classes", type=int, required=True,
                        help="number of label values of the maps: --output_dim of the run, or under --label_regions one more "
                             "than the largest label a SET or VALUE names (4 for 1,2,3=1 2,3=2 3=3)")
    parser.add_argument("--subfolder_prefix", type=str, default="rs", help="rs, pred or native")
    parser.add_argument("--folds", type=int, default=5)
    return parser


def fold_files(in_folder, prefix, folds):
    """-> [(name, [path in fold 0, .., path in fold folds - 1])] for the NIfTI names of Fold0/<prefix>/, sorted"""
    first = os.path.join(in_folder, "Fold0", prefix)
    if not os.path.isdir(first):
        raise SystemExit(f"{first}: no such folder")
    out = []
    for name in sorted(n for n in os.listdir(first) if n.endswith((".nii", ".nii.gz"))):
        paths = [os.path.join(in_folder, "Fold" + str(k), prefix, name) for k in range(folds)]
        for k, p in enumerate(paths):
            if not os.path.isfile(p):
                raise SystemExit(f"{name}: missing in fold {k} ({p})")
        out.append((name, paths))
    return out


def main(args):
    import numpy as np
    import torch

    from medicalsemseg_amd import hip
    from medicalsemseg_amd.utils.nifti import load_nifti, save_nifti
    if args.folds < 1 or args.n_classes < 1:
        raise SystemExit("--folds and --n_classes must be at least 1")
    files = fold_files(args.in_folder, args.subfolder_prefix, args.folds)
    if not torch.cuda.is_available():
        raise SystemExit("majority_vote.py needs an MI355X: medicalsemseg_amd has no CPU fallback")
    out_folder = os.path.join(args.in_folder, "voted_output", args.subfolder_prefix)
    os.makedirs(out_folder, exist_ok=True)
    for name, paths in files:
        maps, affine = [], None
        for k, p in enumerate(paths):
            arr, aff = load_nifti(p)
            if maps and arr.shape != maps[0].shape:
                raise SystemExit(f"{name}: shape {arr.shape} in fold {k}, {maps[0].shape} in fold 0")
            affine = aff if affine is None else affine
            maps.append(np.ascontiguousarray(arr).astype(np.uint8))
        stack = torch.from_numpy(np.stack(maps)).cuda()
        voted = hip.majority_vote_u8(stack, args.n_classes)
        save_nifti(os.path.join(out_folder, name), voted.cpu().numpy(), affine)
    print(f"voted {len(files)} file(s) over {args.folds} fold(s) -> {out_folder}")


if __name__ == "__main__":
    main(build_parser().parse_args())
