"""numpy / scipy restatement of ``msseg_keep_largest_u8`` (MONAI ``KeepLargestConnectedComponent(applied_labels=1..C-1,
is_onehot=False, independent=True)``): per foreground class ``ndimage.label`` with the cross (connectivity 6) or the full
(26) structure, ``bincount``, the FIRST ``argmax`` -- scipy numbers components in raster order of their first voxel, so
among equal sizes the component that starts first is kept -- and everything else of the class becomes 0.  Class 0 and
values >= n_classes are copied and join nothing.  Test-side code only."""
import numpy as np
from scipy import ndimage


def keep_largest_ref(lab: np.ndarray, n_classes: int, connectivity: int = 26):
    """lab uint8 [D, H, W] -> (out uint8 [D, H, W], stats int32 [n_classes, 4] = {components, voxels kept, flat index of
    the kept component's first voxel (-1: class absent), voxels removed}; row 0 is {0, 0, -1, 0})"""
    assert connectivity in (6, 26) and lab.dtype == np.uint8 and lab.ndim == 3
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    out = lab.copy()
    stats = np.zeros((n_classes, 4), np.int32)
    stats[:, 2] = -1
    for c in range(1, n_classes):
        mask = lab == c
        cc, n = ndimage.label(mask, structure=structure)
        if n == 0:
            continue
        sizes = np.bincount(cc.ravel(), minlength=n + 1)[1:]
        k = int(np.argmax(sizes)) + 1                    # first maximum
        out[mask & (cc != k)] = 0
        first = int(np.flatnonzero(cc.ravel() == k)[0])
        stats[c] = (n, sizes[k - 1], first, int(mask.sum()) - int(sizes[k - 1]))
    return out, stats
