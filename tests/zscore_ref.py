"""numpy restatement of the per-volume z-score over the non-zero voxels (--t_zscore / --t_zscore_clip; csrc/volume_stats.hip).
MONAI and nnU-Net are absent: what the tests pin is parity with this file (MONAI parity unpinned).

Per channel of a float32 [C, ...] array:
  1. M = (x != 0) (-0.0 is outside the mask), n = |M|; n == 0 leaves the channel as it is (mean 0, std 1 reported)
  2. with clip (LO, HI): the percentile P_q by numpy's "linear" rule, h = q / 100 * (n - 1), k = floor(h),
     P_q = x_(k) + (h - k) * (x_(min(k + 1, n - 1)) - x_(k)) in double on the two fp32 order statistics, rounded once to fp32;
     y = min(max(x, P_LO), P_HI) on M
  3. mean = sum y / n, std = sqrt(sum (y - mean)^2 / n) in double (population, second pass); a std that is 0 as fp32 -> 1
  4. x = (y - mean) / std on M in fp32 with mean and std rounded once to fp32, one rounding per operation; voxels outside M
     are unchanged
"""
import numpy as np


def ranks_of(q, n):
    """(k, min(k + 1, n - 1), h - k) of the percentage q over n values"""
    h = float(q) / 100.0 * (n - 1)
    k = int(np.floor(h))
    return k, min(k + 1, n - 1), h - k


def percentile_f32(sorted_vals, q):
    """P_q of an ascending float32 array (n >= 1) as float32"""
    s = np.asarray(sorted_vals)
    assert s.dtype == np.float32 and s.ndim == 1 and s.size >= 1
    k, k1, t = ranks_of(q, s.size)
    a, b = float(s[k]), float(s[k1])
    return np.float32(a + t * (b - a))


def channel_stats(x, clip=None):
    """one channel (float32, any shape) -> (n, lo, hi, mean, std): the bounds as float32 (-inf, +inf without clip or with an
    empty mask), mean and std as Python floats (double), std already 1 where it would be 0 as float32"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    m = x != 0
    n = int(m.sum())
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    if n == 0:
        return 0, lo, hi, 0.0, 1.0
    v = x[m]
    if clip is not None:
        s = np.sort(v)
        lo, hi = percentile_f32(s, clip[0]), percentile_f32(s, clip[1])
        v = np.minimum(np.maximum(v, lo), hi)
    v64 = v.astype(np.float64)
    mean = float(v64.sum() / n)
    d = v64 - mean
    std = float(np.sqrt((d * d).sum() / n))
    if np.float32(std) == 0:
        std = 1.0
    return n, lo, hi, mean, std


def apply_channel(x, lo, hi, mean, std):
    """step 4 with the given statistics, each rounded to float32 -> a new float32 array"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    lo, hi, mean, std = (np.float32(v) for v in (lo, hi, mean, std))
    out = x.copy()
    m = x != 0
    y = np.minimum(np.maximum(x[m], lo), hi)
    out[m] = ((y - mean) / std).astype(np.float32)
    return out


def zscore_nonzero(img, clip=None):
    """img float32 [C, ...] -> (the normalised copy, stats float64 [C, 5] = n, lo, hi, mean, std)"""
    img = np.asarray(img)
    out = np.empty_like(img)
    stats = np.zeros((img.shape[0], 5), dtype=np.float64)
    for c in range(img.shape[0]):
        n, lo, hi, mean, std = channel_stats(img[c], clip)
        out[c] = apply_channel(img[c], lo, hi, mean, std)
        stats[c] = (n, lo, hi, mean, std)
    return out, stats
