"""Minimal NIfTI-1 single-file writer / reader (``.nii`` and ``.nii.gz``) for the label maps and volumes the reference
saves with ``nib.save(nib.Nifti1Image(array, affine), path)`` (``/root/reference/engine/test.py:158-170``); nibabel is not
available in this image.  Follows the published NIfTI-1.1 header layout (348 bytes + 4 extension bytes, data at offset
352, little endian): the affine goes to the sform rows with ``sform_code = 2`` (aligned), the quaternion fields are filled
from the same affine with ``qform_code = 0``.  The output is a valid NIfTI-1 file that readers place like the
reference's (same affine, dims, dtype); byte-for-byte equality with nibabel's header is NOT claimed (parity unpinned:
nibabel is absent and no reference fixture holds a header).  Host-side I/O: out of the GPU hot path."""
from __future__ import annotations

import gzip
import struct

import numpy as np

_DTYPES = {np.dtype("uint8"): (2, 8), np.dtype("int16"): (4, 16), np.dtype("int32"): (8, 32), np.dtype("float32"): (16, 32),
           np.dtype("float64"): (64, 64), np.dtype("int8"): (256, 8), np.dtype("uint16"): (512, 16)}
_CODES = {v[0]: k for k, v in _DTYPES.items()}


def _quaternion(R):
    """rotation matrix (det > 0) -> (b, c, d) of the unit quaternion with a >= 0 (NIfTI-1 nifti_mat44_to_quatern)"""
    r11, r12, r13, r21, r22, r23, r31, r32, r33 = R.reshape(-1)
    a = r11 + r22 + r33 + 1.0
    if a > 0.5:
        a = 0.5 * np.sqrt(a)
        b, c, d = 0.25 * (r32 - r23) / a, 0.25 * (r13 - r31) / a, 0.25 * (r21 - r12) / a
    else:
        xd, yd, zd = 1.0 + r11 - (r22 + r33), 1.0 + r22 - (r11 + r33), 1.0 + r33 - (r11 + r22)
        if xd > 1.0:
            b = 0.5 * np.sqrt(xd)
            c, d, a = 0.25 * (r12 + r21) / b, 0.25 * (r13 + r31) / b, 0.25 * (r32 - r23) / b
        elif yd > 1.0:
            c = 0.5 * np.sqrt(yd)
            b, d, a = 0.25 * (r12 + r21) / c, 0.25 * (r23 + r32) / c, 0.25 * (r13 - r31) / c
        else:
            d = 0.5 * np.sqrt(zd)
            b, c, a = 0.25 * (r13 + r31) / d, 0.25 * (r23 + r32) / d, 0.25 * (r21 - r12) / d
        if a < 0.0:
            b, c, d = -b, -c, -d
    return float(b), float(c), float(d)


def save_nifti(path: str, array, affine) -> None:
    a = np.ascontiguousarray(np.asarray(array))
    if a.dtype not in _DTYPES:
        raise ValueError(f"unsupported dtype {a.dtype}")
    if not 1 <= a.ndim <= 7:
        raise ValueError("NIfTI-1 holds 1 to 7 dimensions")
    aff = np.asarray(affine, dtype=np.float64).reshape(4, 4)
    code, bits = _DTYPES[a.dtype]
    dim = [a.ndim] + list(a.shape) + [1] * (7 - a.ndim)
    M = aff[:3, :3]
    vox = np.sqrt((M * M).sum(0))
    vox[vox == 0] = 1.0
    R = M / vox
    qfac = 1.0
    if np.linalg.det(R) < 0:
        R = R.copy()
        R[:, 2] = -R[:, 2]
        qfac = -1.0
    # nearest orthogonal matrix (polar decomposition), as the reference implementation does before the quaternion
    U, _, Vt = np.linalg.svd(R)
    qb, qc, qd = _quaternion(U @ Vt)
    pixdim = [qfac] + [float(v) for v in vox] + [1.0] * 4
    hdr = struct.pack("<i10s18sihcB", 348, b"", b"", 0, 0, b"r", 0)
    hdr += struct.pack("<8h", *dim)
    hdr += struct.pack("<3f", 0.0, 0.0, 0.0)                          # intent_p1..3
    hdr += struct.pack("<4h", 0, code, bits, 0)                       # intent_code, datatype, bitpix, slice_start
    hdr += struct.pack("<8f", *pixdim)
    hdr += struct.pack("<f", 352.0)                                   # vox_offset
    hdr += struct.pack("<2f", float("nan"), float("nan"))             # scl_slope, scl_inter: "no scaling", as nibabel leaves them
    hdr += struct.pack("<hBB", 0, 0, 0)                               # slice_end, slice_code, xyzt_units (unknown: nothing here knows the units)
    hdr += struct.pack("<4f", 0.0, 0.0, 0.0, 0.0)                     # cal_max, cal_min, slice_duration, toffset
    hdr += struct.pack("<2i", 0, 0)                                   # glmax, glmin
    hdr += struct.pack("<80s24s", b"", b"")                           # descrip, aux_file
    hdr += struct.pack("<2h", 0, 2)                                   # qform_code (unknown), sform_code (aligned)
    hdr += struct.pack("<6f", qb, qc, qd, float(aff[0, 3]), float(aff[1, 3]), float(aff[2, 3]))
    hdr += struct.pack("<12f", *[float(v) for v in aff[:3].reshape(-1)])
    hdr += struct.pack("<16s4s", b"", b"n+1\0")
    assert len(hdr) == 348
    # NIfTI stores the first index fastest: Fortran order of the array as nibabel sees it
    payload = hdr + b"\0\0\0\0" + a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes(order="F")
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "wb") as f:
        f.write(payload)


def _quatern_to_mat(b, c, d, qfac, pixdim):
    """NIfTI-1 nifti_quatern_to_mat44: rotation from (b, c, d), columns scaled by pixdim, third column by qfac"""
    a = 1.0 - (b * b + c * c + d * d)
    if a < 1e-7:
        a = 1.0 / np.sqrt(b * b + c * c + d * d)
        b, c, d, a = b * a, c * a, d * a, 0.0
    else:
        a = np.sqrt(a)
    R = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                  [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                  [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]])
    vox = np.array([v if v > 0 else 1.0 for v in pixdim], dtype=np.float64)
    if qfac < 0:
        vox[2] = -vox[2]
    return R * vox[None, :]


def _parse_header(raw):
    """the first 348 bytes of a little-endian single-file NIfTI-1 -> (shape, dtype, data offset, scl_slope, scl_inter, affine)"""
    if len(raw) < 348 or struct.unpack("<i", raw[:4])[0] != 348 or raw[344:348] != b"n+1\0":
        raise ValueError("not a little-endian single-file NIfTI-1")
    dim = struct.unpack("<8h", raw[40:56])
    code, bits = struct.unpack("<2h", raw[70:74])
    pixdim = struct.unpack("<8f", raw[76:108])
    off = int(struct.unpack("<f", raw[108:112])[0])
    slope, inter = struct.unpack("<2f", raw[112:120])
    qform_code, sform_code = struct.unpack("<2h", raw[252:256])
    shape = dim[1:1 + dim[0]]
    if code not in _CODES:
        raise ValueError(f"unsupported NIfTI datatype code {code}")
    dt = _CODES[code].newbyteorder("<")
    aff = np.eye(4)
    if sform_code > 0:
        aff[:3] = np.array(struct.unpack("<12f", raw[280:328])).reshape(3, 4)
    elif qform_code > 0:
        b, c, d, qx, qy, qz = struct.unpack("<6f", raw[256:280])
        aff[:3, :3] = _quatern_to_mat(b, c, d, pixdim[0], pixdim[1:4])
        aff[:3, 3] = (qx, qy, qz)
    else:
        aff[:3, :3] = np.diag([v if v > 0 else 1.0 for v in pixdim[1:4]])
    return shape, dt, off, slope, inter, aff


def read_nifti_header(path: str):
    """-> (shape, affine) as load_nifti gives them, from the header alone (a .gz is inflated only that far)"""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = f.read(348)
    shape, _, _, _, _, aff = _parse_header(raw)
    return tuple(shape), aff


def load_nifti(path: str):
    """-> (array, affine).  Reads little-endian single-file NIfTI-1: up to 7 dimensions (a 4-D file keeps its channels
    last), ``scl_slope`` / ``scl_inter`` applied (-> float32) when the slope is finite and non-zero and the pair is not the
    identity, affine from the sform rows when ``sform_code > 0``, else from the qform quaternion and ``pixdim`` when
    ``qform_code > 0``, else ``diag(pixdim)``.  What save_nifti writes reads back unchanged."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        raw = f.read()
    shape, dt, off, slope, inter, aff = _parse_header(raw)
    data = np.frombuffer(raw, dtype=dt, count=int(np.prod(shape)), offset=off).reshape(shape, order="F")
    if np.isfinite(slope) and slope != 0.0 and np.isfinite(inter) and not (slope == 1.0 and inter == 0.0):
        data = data.astype(np.float32) * np.float32(slope) + np.float32(inter)
    return data, aff
