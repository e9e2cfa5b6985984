"""numpy restatement of msseg_restore_native_u8 (include/msseg.h): the same IEEE operations in the same order -- float64
coordinates, float32 lerps a + f * (b - a) through np.float32 arithmetic along model axis 2, 1, 0, first strictly greatest
channel -- so a comparison with the kernel is exact equality of uint8 maps.  The descriptor is a plain dict with the
fields of msseg_restore_desc; desc_of() reads one off a ctypes RestoreDesc."""
import numpy as np

FIELDS = ("native", "perm", "flip", "grid", "offset", "model", "scale")


def desc_of(d):
    """hip.RestoreDesc (or a dict) -> dict of tuples"""
    if isinstance(d, dict):
        return {k: tuple(d[k]) for k in FIELDS}
    return {k: tuple(getattr(d, k)) for k in FIELDS}


def make_desc(native, perm=(0, 1, 2), flip=(0, 0, 0), grid=None, offset=(0, 0, 0), model=None, scale=(1.0, 1.0, 1.0)):
    oriented = tuple(native[p] for p in perm)
    grid = oriented if grid is None else tuple(grid)
    return {"native": tuple(native), "perm": tuple(perm), "flip": tuple(int(bool(f)) for f in flip), "grid": grid,
            "offset": tuple(offset), "model": grid if model is None else tuple(model), "scale": tuple(float(s) for s in scale)}


def axis_coords(desc, k):
    """oriented axis k -> m (float64 [native[perm[k]]]): the model coordinate of every index of that native axis"""
    n = desc["native"][desc["perm"][k]]
    o = np.arange(n, dtype=np.int64)
    if desc["flip"][k]:
        o = n - 1 - o
    s = o.astype(np.float64) * np.float64(desc["scale"][k])
    s = np.where(s > np.float64(desc["grid"][k] - 1), np.float64(desc["grid"][k] - 1), s)
    return s + np.float64(desc["offset"][k])


def _native_view(arrs, desc):
    """per oriented axis a 1-D array over its native axis -> the three arrays shaped to broadcast over [native]"""
    out = []
    for k in range(3):
        shape = [1, 1, 1]
        shape[desc["perm"][k]] = -1
        out.append(np.asarray(arrs[k]).reshape(shape))
    return out


def restore_ref(src, desc, mode="nearest"):
    """src uint8 [model] (nearest) or float32 [C][model] (linear) -> uint8 [native]"""
    desc = desc_of(desc)
    model = desc["model"]
    m = [axis_coords(desc, k) for k in range(3)]
    q = [np.floor(m[k] + 0.5) for k in range(3)]
    inside = [(q[k] >= 0) & (q[k] < model[k]) for k in range(3)]
    I0, I1, I2 = _native_view(inside, desc)
    air = ~(I0 & I1 & I2)
    if mode == "nearest":
        assert src.dtype == np.uint8 and src.shape == tuple(model)
        qi = [np.clip(q[k], 0, model[k] - 1).astype(np.int64) for k in range(3)]
        Q0, Q1, Q2 = _native_view(qi, desc)
        out = src[Q0, Q1, Q2]
        return np.where(air, np.uint8(0), out).astype(np.uint8)
    assert mode == "linear" and src.dtype == np.float32 and src.shape[1:] == tuple(model)
    i0 = [np.floor(m[k]) for k in range(3)]
    f = [(m[k] - i0[k]).astype(np.float32) for k in range(3)]
    lo = [np.clip(i0[k], 0, model[k] - 1).astype(np.int64) for k in range(3)]
    hi = [np.clip(i0[k] + 1, 0, model[k] - 1).astype(np.int64) for k in range(3)]
    L0, L1, L2 = _native_view(lo, desc)
    H0, H1, H2 = _native_view(hi, desc)
    F0, F1, F2 = _native_view(f, desc)
    best, out = None, np.zeros(desc["native"], dtype=np.uint8)
    for c in range(src.shape[0]):
        s = src[c]

        def lerp(a, b, w):
            return (a + w * (b - a)).astype(np.float32)       # float32 operands: every operation rounds to float32
        v00 = lerp(s[L0, L1, L2], s[L0, L1, H2], F2)
        v01 = lerp(s[L0, H1, L2], s[L0, H1, H2], F2)
        v10 = lerp(s[H0, L1, L2], s[H0, L1, H2], F2)
        v11 = lerp(s[H0, H1, L2], s[H0, H1, H2], F2)
        v = lerp(lerp(v00, v01, F1), lerp(v10, v11, F1), F0)
        assert v.dtype == np.float32
        if c == 0:
            best = v.copy()
        else:
            better = v > best
            best = np.where(better, v, best)
            out[better] = c
    return np.where(air, np.uint8(0), out).astype(np.uint8)


def restore_by_construction(lab, desc):
    """unit scale only, nearest: the inverse chain by plain array steps -- un-pad, place the crop into a zero array at the
    box, un-flip, inverse transpose.  Independent of restore_ref's coordinate arithmetic."""
    desc = desc_of(desc)
    assert all(s == 1.0 for s in desc["scale"])
    grid, model, off = desc["grid"], desc["model"], desc["offset"]
    full = np.zeros(grid, dtype=np.uint8)
    # grid index g sits at model index g + offset: copy the overlap of [0, grid) with [-offset, model - offset)
    g_lo = [max(0, -off[k]) for k in range(3)]
    g_hi = [min(grid[k], model[k] - off[k]) for k in range(3)]
    if all(g_hi[k] > g_lo[k] for k in range(3)):
        full[g_lo[0]:g_hi[0], g_lo[1]:g_hi[1], g_lo[2]:g_hi[2]] = \
            lab[g_lo[0] + off[0]:g_hi[0] + off[0], g_lo[1] + off[1]:g_hi[1] + off[1], g_lo[2] + off[2]:g_hi[2] + off[2]]
    for k in range(3):
        if desc["flip"][k]:
            full = np.flip(full, axis=k)
    return np.ascontiguousarray(np.transpose(full, np.argsort(desc["perm"])))


def majority_vote_ref(maps, n_classes):
    """maps: uint8 [F][...] -> one vote per fold for its foreground class, background starts with one vote, first maximum"""
    maps = np.asarray(maps)
    votes = np.zeros((n_classes,) + maps.shape[1:], dtype=np.int64)
    for c in range(1, n_classes):
        votes[c] = (maps == c).sum(0)
    votes[0] += 1
    return np.argmax(votes, axis=0).astype(np.uint8)


ORIENTATIONS = [(p, (a, b, c)) for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
                for a in (0, 1) for b in (0, 1) for c in (0, 1)]
