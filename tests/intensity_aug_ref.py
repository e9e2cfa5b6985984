"""numpy / scipy float64 restatement of msseg_intensity_aug (include/msseg.h, csrc/intensity_aug.hip): noise -> blur ->
contrast -> gamma on the inverted image -> gamma, per (patch, channel) row, and the uint32 restatement of the noise
generator's integer stage (Philox4x32-10).  Used by tests/test_intensity_aug_host.py and tests/test_gpu_intensity_aug.py."""
import numpy as np

NOISE, BLUR, CONTRAST, GAMMA_INV, GAMMA = 1, 2, 4, 8, 16
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def _mulhilo(m, c):
    p = np.uint64(m) * c.astype(np.uint64)
    return (p >> np.uint64(32)).astype(np.uint32), (p & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def philox4x32_10(counter, key):
    """counter: uint32 [n, 4], key: (k0, k1) -> uint32 [n, 4]; every intermediate is a uint32 (the 32 x 32 -> 64 bit product is
    split into its halves at once)"""
    c = [np.ascontiguousarray(counter[:, j]).astype(np.uint32) for j in range(4)]
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c[0])
        hi1, lo1 = _mulhilo(_M1, c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = np.uint32((int(k0) + _W0) & 0xFFFFFFFF)
        k1 = np.uint32((int(k1) + _W1) & 0xFFFFFFFF)
    return np.stack(c, axis=1)


def noise_words(key, n, first=0):
    """the four words of the voxel indices first .. first + n - 1 under a 64-bit key: counter {index lo, index hi, 0, 0}"""
    i = np.arange(first, first + n, dtype=np.uint64)
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (i >> np.uint64(32)).astype(np.uint32)
    return philox4x32_10(ctr, (int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF))


def uniforms(words):
    """((bits >> 8) + 0.5) * 2^-24 evaluated in fp32 as the kernel does (values of 0.5 and above round to a multiple of
    2^-24 there, 1.0 included; never 0), returned as float64"""
    w = (words >> np.uint32(8)).astype(np.float32)
    return ((w + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)


def normals(key, n, first=0):
    """float64 Box-Muller (cosine branch) of the kernel's uniforms"""
    w = noise_words(key, n, first)
    u1, u2 = uniforms(w[:, 0]), uniforms(w[:, 1])
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def blur(x, sigma):
    """scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4) restated: radius int(4 sigma + 0.5), weights
    exp(-k^2 / (2 sigma^2)) normalised, reflection d c b a | a b c d | d c b a, all three axes"""
    x = np.asarray(x, dtype=np.float64)
    sigma = float(sigma)
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (sigma * sigma))
    w /= w.sum()
    for axis in range(3):
        n = x.shape[axis]
        idx = np.arange(-r, n + r)
        idx = np.where(idx < 0, -idx - 1, np.where(idx >= n, 2 * n - 1 - idx, idx))
        p = np.take(x, idx, axis=axis)
        x = sum(w[j] * np.take(p, np.arange(j, j + n), axis=axis) for j in range(2 * r + 1))
    return x


def contrast(x, f):
    x = np.asarray(x, dtype=np.float64)
    m, lo, hi = x.mean(), x.min(), x.max()
    return np.clip((x - m) * f + m, lo, hi)


def gamma(x, g, invert=False):
    """retain-statistics gamma; invert: the same on -x, negated back"""
    x = np.asarray(x, dtype=np.float64)
    if invert:
        return -gamma(-x, g)
    m, s, lo = x.mean(), x.std(), x.min()
    R = x.max() - lo
    y = np.power((x - lo) / (R + 1e-7), g) * R + lo
    return (y - y.mean()) / (y.std() + 1e-8) * s + m


def apply_row(x, row):
    """one (patch, channel) volume x [D, H, W] under a row with the fields of msseg_intensity_row -> float64"""
    x = np.asarray(x, dtype=np.float64)
    if row.mask & NOISE:
        x = x + float(np.float32(row.noise_std)) * normals(row.noise_key, x.size).reshape(x.shape)
    if row.mask & BLUR:
        x = blur(x, float(np.float32(row.blur_sigma)))
    if row.mask & CONTRAST:
        x = contrast(x, float(np.float32(row.contrast)))
    if row.mask & GAMMA_INV:
        x = gamma(x, float(np.float32(row.gamma_inv)), invert=True)
    if row.mask & GAMMA:
        x = gamma(x, float(np.float32(row.gamma)))
    return x


def apply(batch, rows):
    """batch [N, C, D, H, W], rows in order n * C + c -> float64"""
    batch = np.asarray(batch)
    out = np.empty(batch.shape, dtype=np.float64)
    N, C = batch.shape[:2]
    for n in range(N):
        for c in range(C):
            out[n, c] = apply_row(batch[n, c], rows[n * C + c])
    return out
