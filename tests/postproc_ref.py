"""numpy / scipy restatement of ``msseg_postprocess_u8``: three optional steps on a uint8 label map, always in this order.

1. ``min_size = N`` (0, 1: off): per foreground class ``ndimage.label`` with the cross (connectivity 6) or the full (26)
   structure; every component with fewer than N voxels becomes 0 (MONAI ``RemoveSmallObjects``, nnU-Net).
2. ``keep_largest``: ``tests/components_ref.keep_largest_ref`` on what step 1 left.
3. ``fill_holes``: for c = 1, 2, .., C-1 in this order, each on the map the class before left,
   ``out[ndimage.binary_fill_holes(out == c, structure)] = c`` with the structure of ``hole_connectivity``: scipy dilates
   the outside into the complement of the class with that structure, so it is the connectivity of the leak path.
   ``fill_holes_dilation_ref`` is MONAI ``FillHoles``' form of the same step.

Class 0 and values >= n_classes are copied by steps 1 and 2 and join nothing; step 3 overwrites them where enclosed.
Test-side code only."""
import numpy as np
from scipy import ndimage

from tests.components_ref import keep_largest_ref


def _structure(connectivity: int):
    assert connectivity in (6, 26)
    return ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)


def fill_holes_ref(lab: np.ndarray, n_classes: int, hole_connectivity: int = 26):
    """-> (out, voxels turned into each class by its own fill step: int list of n_classes entries)"""
    st = _structure(hole_connectivity)
    out = lab.copy()
    filled = [0] * n_classes
    for c in range(1, n_classes):
        mask = out == c
        full = ndimage.binary_fill_holes(mask, structure=st)
        filled[c] = int(full.sum()) - int(mask.sum())
        out[full] = c
    return out, filled


def fill_holes_dilation_ref(lab: np.ndarray, n_classes: int, hole_connectivity: int = 26):
    """the same step as MONAI ``FillHoles`` writes it: flood the complement of the class from outside the volume
    (``border_value=1``) and fill what the flood does not reach"""
    st = _structure(hole_connectivity)
    out = lab.copy()
    for c in range(1, n_classes):
        outside = ndimage.binary_dilation(np.zeros(out.shape, bool), structure=st, iterations=-1, mask=out != c,
                                          border_value=1)
        out[~outside] = c
    return out


def postprocess_ref(lab: np.ndarray, n_classes: int, min_size: int = 0, keep_largest: bool = False, connectivity: int = 26,
                    fill_holes: bool = False, hole_connectivity: int = 26):
    """lab uint8 [D, H, W] -> (out uint8 [D, H, W], stats int32 [n_classes, 6] = {components before any step (-1 when
    neither step 1 nor step 2 is on: the classes are then not labelled), components removed as small, voxels removed as
    small, voxels removed by keep-largest, voxels turned into the class by its fill step, voxels of the class in the final
    map}; row 0 is all zero)"""
    assert lab.dtype == np.uint8 and lab.ndim == 3 and min_size >= 0
    st = _structure(connectivity)
    _structure(hole_connectivity)
    out = lab.copy()
    stats = np.zeros((n_classes, 6), np.int32)
    labelled = min_size > 1 or keep_largest
    for c in range(1, n_classes):
        if not labelled:
            stats[c, 0] = -1
            continue
        cc, n = ndimage.label(lab == c, structure=st)
        stats[c, 0] = n
        sizes = np.bincount(cc.ravel(), minlength=n + 1)
        small = np.flatnonzero(sizes[1:] < min_size) + 1
        stats[c, 1] = len(small)
        stats[c, 2] = int(sizes[small].sum())
        out[np.isin(cc, small)] = 0
    if keep_largest:
        out, kl = keep_largest_ref(out, n_classes, connectivity)
        stats[:, 3] = kl[:, 3]
    if fill_holes:
        out, filled = fill_holes_ref(out, n_classes, hole_connectivity)
        stats[:, 4] = filled
    for c in range(1, n_classes):
        stats[c, 5] = int((out == c).sum())
    return out, stats
