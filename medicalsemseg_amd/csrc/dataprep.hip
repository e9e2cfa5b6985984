// Dataset path on the device: one-off preprocessing of a loaded volume and the per-step multi-volume patch gather.
//
//   intensity_prep    ScaleIntensityRanged / ScaleCubedIntensityRanged (+ NormalizeIntensityd) and, in the same pass,
//                     the bounding box CropForegroundd(source_key="image") selects
//                     (data/dataset_builder.py:37-81,194-210, data/transforms.py:45-75)
//   resample_spacing  Spacingd(pixdim, mode=("bilinear", "nearest"))            (dataset_builder.py:30-36)
//   crop_pad_copy     CropForegroundd's crop + SpatialPadd(vol_size)            (dataset_builder.py:69-87)
//   slab_counts       per z-slice numbers of the crop-centre candidates RandCropByPosNegLabeld draws from (:108-120);
//                     the image side of a background candidate is `> threshold` or, for a z-scored cache, `!= threshold`
//   pick_voxels       the k-th candidate of a slice -> crop centre (correct_crop_centers clamp) and crop start; the scan
//                     lives in pick_scan.h, which class_crop.hip shares
//   aug_crop_multi    msseg_aug_crop_batch over many cached volumes: one launch per batch
//   aug_crop_affine   aug_crop_multi sampling the volume under a 3x3 matrix per patch (rotation + zoom about the patch centre)
//
// MONAI is absent: the semantics are those of the numpy / scipy restatement in tests/dataprep_ref.py (MONAI parity
// unpinned).  All kernels are HBM-bound; geometry (z, y) comes from the launch grid, threads run along x.
#include "common.h"
#include "pick_scan.h"

namespace {

using pick::VolDesc;
using pick::PickRow;
using pick::bg_image_ok;

typedef float f32x4u_t __attribute__((ext_vector_type(4), aligned(4)));

MSSEG_DEVFN int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
MSSEG_DEVFN int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

__global__ void box_init_kernel(int* box6, int D, int H, int W) {
    const int t = threadIdx.x;
    if (t < 6) box6[t] = t == 0 ? D : (t == 1 ? H : (t == 2 ? W : -1));
}

// grid: (x blocks, H, D); every thread one x of one (z, y) row, all channels
template <typename TS>
__global__ __launch_bounds__(256) void intensity_prep_kernel(const TS* __restrict__ src, int C, int D, int H, int W, int mode,
                                                             float a_min, float a_range, int normalize, float sub, float dv,
                                                             float* __restrict__ dst, int* __restrict__ box6) {
#pragma clang fp contract(off)   // one rounding per numpy operation
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    const long long V = (long long)D * H * W;
    bool fg = false;
    if (x < W) {
        const long long v = ((long long)z * H + y) * W + x;
        for (int c = 0; c < C; ++c) {
            float t = (float)src[(long long)c * V + v];
            if (mode != 0) {
                if (mode == 2) t = cbrtf(t);
                t = (t - a_min) / a_range;
                t = t * 1.0f + 0.0f;                       // * (b_max - b_min) + b_min with the reference's (0, 1)
                t = fminf(fmaxf(t, 0.0f), 1.0f);
            }
            fg = fg || t > 0.0f;
            if (normalize) t = (t - sub) / dv;
            dst[(long long)c * V + v] = t;
        }
    }
    // box of the foreground voxels: (z, y) are uniform over the block, x is reduced per wave
    const int xmin = wave_min_i(fg ? x : 0x7fffffff), xmax = wave_max_i(fg ? x : -1);
    if ((threadIdx.x & 63) == 0 && xmax >= 0) {
        atomicMin(box6 + 0, z); atomicMin(box6 + 1, y); atomicMin(box6 + 2, xmin);
        atomicMax(box6 + 3, z); atomicMax(box6 + 4, y); atomicMax(box6 + 5, xmax);
    }
}

// grid: (x blocks, TH, TD).  Source coordinate = destination index * (new spacing / old spacing), in double.
template <bool LABEL>
__global__ __launch_bounds__(256) void resample_spacing_kernel(const void* __restrict__ src_, int C, int SD, int SH, int SW,
                                                               void* __restrict__ dst_, int TD, int TH, int TW, double rz,
                                                               double ry, double rx) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= TW) return;
    const long long SV = (long long)SD * SH * SW, TV = (long long)TD * TH * TW;
    const long long o = ((long long)z * TH + y) * TW + x;
    double cz = (double)z * rz, cy = (double)y * ry, cx = (double)x * rx;
    if constexpr (LABEL) {
        const unsigned char* src = (const unsigned char*)src_;
        unsigned char* dst = (unsigned char*)dst_;
        int iz = (int)floor(cz + 0.5), iy = (int)floor(cy + 0.5), ix = (int)floor(cx + 0.5);
        iz = iz < 0 ? 0 : (iz > SD - 1 ? SD - 1 : iz);
        iy = iy < 0 ? 0 : (iy > SH - 1 ? SH - 1 : iy);
        ix = ix < 0 ? 0 : (ix > SW - 1 ? SW - 1 : ix);
        for (int c = 0; c < C; ++c) dst[(long long)c * TV + o] = src[(long long)c * SV + ((long long)iz * SH + iy) * SW + ix];
    } else {
        const float* src = (const float*)src_;
        float* dst = (float*)dst_;
        cz = cz < 0.0 ? 0.0 : (cz > (double)(SD - 1) ? (double)(SD - 1) : cz);
        cy = cy < 0.0 ? 0.0 : (cy > (double)(SH - 1) ? (double)(SH - 1) : cy);
        cx = cx < 0.0 ? 0.0 : (cx > (double)(SW - 1) ? (double)(SW - 1) : cx);
        const int z0 = (int)floor(cz), y0 = (int)floor(cy), x0 = (int)floor(cx);
        const int z1 = z0 + 1 < SD ? z0 + 1 : SD - 1, y1 = y0 + 1 < SH ? y0 + 1 : SH - 1, x1 = x0 + 1 < SW ? x0 + 1 : SW - 1;
        const float fz = (float)(cz - (double)z0), fy = (float)(cy - (double)y0), fx = (float)(cx - (double)x0);
        const long long r00 = ((long long)z0 * SH + y0) * SW, r01 = ((long long)z0 * SH + y1) * SW;
        const long long r10 = ((long long)z1 * SH + y0) * SW, r11 = ((long long)z1 * SH + y1) * SW;
        for (int c = 0; c < C; ++c) {
            const float* s = src + (long long)c * SV;
            // a + f * (b - a): a zero fraction returns the sample itself (identity spacing copies bit for bit)
            const float v00 = s[r00 + x0] + fx * (s[r00 + x1] - s[r00 + x0]);
            const float v01 = s[r01 + x0] + fx * (s[r01 + x1] - s[r01 + x0]);
            const float v10 = s[r10 + x0] + fx * (s[r10 + x1] - s[r10 + x0]);
            const float v11 = s[r11 + x0] + fx * (s[r11 + x1] - s[r11 + x0]);
            const float v0 = v00 + fy * (v01 - v00), v1 = v10 + fy * (v11 - v10);
            dst[(long long)c * TV + o] = v0 + fz * (v1 - v0);
        }
    }
}

// grid: (x blocks, TH, TD); dst[c][z][y][x] = src[c][z0 + z - pz][..][..] inside the box, pad elsewhere
template <typename T>
__global__ __launch_bounds__(256) void crop_pad_copy_kernel(const T* __restrict__ src, int C, int SD, int SH, int SW, int z0,
                                                            int y0, int x0, int bd, int bh, int bw, T* __restrict__ dst, int TD,
                                                            int TH, int TW, int pz, int py, int px, T pad) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= TW) return;
    const long long SV = (long long)SD * SH * SW, TV = (long long)TD * TH * TW;
    const int bz = z - pz, by = y - py, bx = x - px;
    const bool in = bz >= 0 && bz < bd && by >= 0 && by < bh && bx >= 0 && bx < bw;
    const long long s = ((long long)(z0 + bz) * SH + (y0 + by)) * SW + (x0 + bx), o = ((long long)z * TH + y) * TW + x;
    for (int c = 0; c < C; ++c) dst[(long long)c * TV + o] = in ? src[(long long)c * SV + s] : pad;
}

// one block per z-slice; counts[z] = {#(lab > 0), #(lab == 0 && bg_image_ok(img0))}
__global__ __launch_bounds__(256) void slab_counts_kernel(const float* __restrict__ img0, const unsigned char* __restrict__ lab,
                                                          int HW, float thr, int rule, int* __restrict__ counts) {
    __shared__ int sfg[4], sbg[4];
    const long long base = (long long)blockIdx.x * HW;
    int fg = 0, bg = 0;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const unsigned char l = lab[base + i];
        fg += l > 0;
        bg += (l == 0 && bg_image_ok(img0[base + i], thr, rule));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { fg += __shfl_xor(fg, o); bg += __shfl_xor(bg, o); }
    if ((threadIdx.x & 63) == 0) { sfg[threadIdx.x >> 6] = fg; sbg[threadIdx.x >> 6] = bg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[2 * blockIdx.x + 0] = sfg[0] + sfg[1] + sfg[2] + sfg[3];
        counts[2 * blockIdx.x + 1] = sbg[0] + sbg[1] + sbg[2] + sbg[3];
    }
}

// one block per row: counting scan (pick_scan.h) of slice `z` of volume `vol` in flat order
__global__ __launch_bounds__(256) void pick_voxels_kernel(const VolDesc* __restrict__ vols, int nvol,
                                                          const PickRow* __restrict__ rows, int R, float thr,
                                                          int rule, int* __restrict__ out) {
    __shared__ int scan[256];
    __shared__ int found;
    const PickRow row = rows[blockIdx.x];
    int* o = out + 8 * blockIdx.x;
    if (row.vol < 0 || row.vol >= nvol) {
        if (threadIdx.x < 8) o[threadIdx.x] = threadIdx.x < 6 ? 0 : -1;
        return;
    }
    const VolDesc vd = vols[row.vol];
    const int HW = vd.H * vd.W;
    const int z = row.z < 0 ? 0 : (row.z >= vd.D ? vd.D - 1 : row.z);
    int hit;
    if (row.mode == 2) {
        hit = row.rank < 0 ? 0 : (row.rank >= HW ? HW - 1 : row.rank);      // explicit voxel of the slice
    } else {
        const pick::FgBgPred pred{vd.lab + (long long)z * HW, vd.img + (long long)z * HW, thr, rule, row.mode == 1};
        hit = pick::scan_slice(HW, row.rank, pred, scan, &found);
    }
    if (threadIdx.x == 0) pick::write_pick(o, vd, z, hit, R);
}

// Row prologue shared by the two crop gathers below; (z, y) is the thread's output row of patch b.
// *vd = the row's volume; true when the patch can be read from it.  A row that names no volume, or a volume that cannot
// hold the patch: this thread's share of a defined all-zero patch is written, nothing is read, and the answer is false.
template <typename TO>
MSSEG_DEVFN bool crop_row_volume(const VolDesc* __restrict__ vols, int nvol, const PickRow& row, int b, int z, int y,
                                 TO* __restrict__ out_img, float* __restrict__ out_lab, int C, int R, VolDesc* vd) {
    const bool known = row.vol >= 0 && row.vol < nvol;
    *vd = vols[known ? row.vol : 0];
    if (known && vd->C == C && R <= vd->D && R <= vd->H && R <= vd->W) return true;
    const long long R3 = (long long)R * R * R, orow = ((long long)z * R + y) * R;
    for (int x = threadIdx.x; x < R; x += blockDim.x) {
        for (int c = 0; c < C; ++c) DT<TO>::st(out_img + ((long long)b * C + c) * R3 + orow + x, 0.0f);
        out_lab[(long long)b * R3 + orow + x] = 0.0f;
    }
    return false;
}

// crop start from the pick table, kept inside the volume whatever the table holds
MSSEG_DEVFN void crop_start(const int* __restrict__ picks, int b, const VolDesc& vd, int R, int* z0, int* y0, int* x0) {
    const int pz = picks[8 * b + 3], py = picks[8 * b + 4], px = picks[8 * b + 5];
    *z0 = pz < 0 ? 0 : (pz > vd.D - R ? vd.D - R : pz);
    *y0 = py < 0 ? 0 : (py > vd.H - R ? vd.H - R : py);
    *x0 = px < 0 ? 0 : (px > vd.W - R ? vd.W - R : px);
}

// patch index (sz, sy) of output row (z, y): rot90^k in the (z, y) plane undone -- out[i, j] = m[j, n-1-i] (k = 1),
// m[n-1-i, n-1-j] (2), m[n-1-j, i] (3) -- then the flips along z and y; the flip along x is left to the caller's x loop
MSSEG_DEVFN void patch_row_index(const PickRow& row, int z, int y, int R, int* sz, int* sy) {
    *sz = z; *sy = y;
    if (row.rotk == 1) { *sz = y; *sy = R - 1 - z; }
    else if (row.rotk == 2) { *sz = R - 1 - z; *sy = R - 1 - y; }
    else if (row.rotk == 3) { *sz = R - 1 - y; *sy = z; }
    if (row.flips & 1) *sz = R - 1 - *sz;
    if (row.flips & 2) *sy = R - 1 - *sy;
}

// grid: (y tiles, R, npatch), block (runs of 4 along x, rows).  Every thread moves runs of 4 consecutive output x.
template <typename TO>
__global__ __launch_bounds__(256) void aug_crop_multi_kernel(const VolDesc* __restrict__ vols, int nvol,
                                                             const PickRow* __restrict__ rows, const int* __restrict__ picks,
                                                             TO* __restrict__ out_img, float* __restrict__ out_lab, int C, int R) {
#pragma clang fp contract(off)   // (v + shift) * scale with two roundings, as the two numpy transforms apply them
    const int b = blockIdx.z, z = blockIdx.y, y = blockIdx.x * blockDim.y + threadIdx.y;
    if (y >= R) return;
    const PickRow row = rows[b];
    VolDesc vd;
    if (!crop_row_volume(vols, nvol, row, b, z, y, out_img, out_lab, C, R, &vd)) return;
    int z0, y0, x0, sz, sy;
    crop_start(picks, b, vd, R, &z0, &y0, &x0);
    patch_row_index(row, z, y, R, &sz, &sy);
    const bool fx = (row.flips & 4) != 0;
    const long long V = (long long)vd.D * vd.H * vd.W, R3 = (long long)R * R * R;
    const long long srow = ((long long)(z0 + sz) * vd.H + (y0 + sy)) * vd.W + x0;
    const long long orow = ((long long)z * R + y) * R;
    const bool vec = (R & 3) == 0;
    for (int x = threadIdx.x * 4; x < R; x += blockDim.x * 4) {
        const int n = R - x < 4 ? R - x : 4;
        const int sx = fx ? R - x - n : x;                                   // first source x of the run
        if (vec) {
            for (int c = 0; c < C; ++c) {
                f32x4_t v = *(const f32x4u_t*)(vd.img + (long long)c * V + srow + sx);
                if (fx) v = f32x4_t{v[3], v[2], v[1], v[0]};
                v = (v + row.shift) * row.scale;
                const float o[4] = {v[0], v[1], v[2], v[3]};
                store4<TO>(out_img + ((long long)b * C + c) * R3 + orow + x, o);
            }
            if (vd.lab) {
                const unsigned char* l = vd.lab + srow + sx;
                f32x4_t v = {(float)l[0], (float)l[1], (float)l[2], (float)l[3]};
                if (fx) v = f32x4_t{v[3], v[2], v[1], v[0]};
                *(f32x4_t*)(out_lab + (long long)b * R3 + orow + x) = v;
            }
        } else {
            for (int e = 0; e < n; ++e) {
                const int se = fx ? sx + n - 1 - e : sx + e;
                for (int c = 0; c < C; ++c) {
                    const float a = vd.img[(long long)c * V + srow + se] + row.shift;
                    DT<TO>::st(out_img + ((long long)b * C + c) * R3 + orow + x + e, a * row.scale);
                }
                if (vd.lab) out_lab[(long long)b * R3 + orow + x + e] = (float)vd.lab[srow + se];
            }
        }
    }
}

// floor(c) (image, lo = -2) or floor(c + 0.5) (label, lo = -1) as an index that is safe to test against [0, n) and to add
// 1 to, whatever the matrix table holds: values beyond the volume collapse onto lo / n, a NaN onto lo
MSSEG_DEVFN int affine_index(double fl, double lo, int n) { return (int)fmin(fmax(fl, lo), (double)n); }

// grid: (y tiles, R, npatch), block (32 along x, 8 rows).  The patch row, its matrix and the crop start are uniform per
// block.  Source coordinate of patch index p, about the patch's geometric centre: c = (start + h) + M (p - h), h = (R - 1) / 2,
// in double; image = trilinear over 8 taps (a tap outside the volume reads `pad`: scipy's mode="grid-constant"), fp32 lerps
// a + f * (b - a) along x, y, z as resample_spacing_kernel; label = the nearest voxel floor(c + 0.5), 0 outside.
// No LDS staging: the 32 x 8 voxels of a block map onto a slanted slab of a few KiB of the source, which the taps of
// neighbouring lanes and rows re-read from the CU's vector cache; coordinates and fractions are shared by the C channels.
template <typename TO>
__global__ __launch_bounds__(256) void aug_crop_affine_kernel(const VolDesc* __restrict__ vols, int nvol,
                                                              const PickRow* __restrict__ rows, const int* __restrict__ picks,
                                                              const double* __restrict__ mats, TO* __restrict__ out_img,
                                                              float* __restrict__ out_lab, int C, int R, float pad) {
#pragma clang fp contract(off)   // every product and sum of the coordinate and of the lerps rounds once, in the stated order
    const int b = blockIdx.z, z = blockIdx.y, y = blockIdx.x * blockDim.y + threadIdx.y;
    if (y >= R) return;
    const PickRow row = rows[b];
    VolDesc vd;
    if (!crop_row_volume(vols, nvol, row, b, z, y, out_img, out_lab, C, R, &vd)) return;
    int z0, y0, x0, sz, sy;
    crop_start(picks, b, vd, R, &z0, &y0, &x0);
    patch_row_index(row, z, y, R, &sz, &sy);
    const long long R3 = (long long)R * R * R, orow = ((long long)z * R + y) * R;
    const bool flipx = (row.flips & 4) != 0;
    const double* M = mats + 9 * (long long)b;
    const double h = (double)(R - 1) / 2.0;
    const double dz = (double)sz - h, dy = (double)sy - h;
    const double bz = (double)z0 + h, by = (double)y0 + h, bx = (double)x0 + h;
    const double pz = M[0] * dz + M[1] * dy, py = M[3] * dz + M[4] * dy, px = M[6] * dz + M[7] * dy;
    const long long HW = (long long)vd.H * vd.W, V = (long long)vd.D * HW;
    for (int x = threadIdx.x; x < R; x += blockDim.x) {
        const double dx = (double)(flipx ? R - 1 - x : x) - h;
        const double cz = bz + (pz + M[2] * dx), cy = by + (py + M[5] * dx), cx = bx + (px + M[8] * dx);
        const double lz = floor(cz), ly = floor(cy), lx = floor(cx);
        const float wz = (float)(cz - lz), wy = (float)(cy - ly), wx = (float)(cx - lx);
        const int iz = affine_index(lz, -2.0, vd.D), iy = affine_index(ly, -2.0, vd.H), ix = affine_index(lx, -2.0, vd.W);
        const bool z0in = iz >= 0 && iz < vd.D, z1in = iz + 1 >= 0 && iz + 1 < vd.D;
        const bool y0in = iy >= 0 && iy < vd.H, y1in = iy + 1 >= 0 && iy + 1 < vd.H;
        const bool x0in = ix >= 0 && ix < vd.W, x1in = ix + 1 >= 0 && ix + 1 < vd.W;
        const long long o = (long long)iz * HW + (long long)iy * vd.W + ix;            // read only where the tap is inside
        for (int c = 0; c < C; ++c) {
            const float* s = vd.img + (long long)c * V + o;
            const float t000 = z0in && y0in && x0in ? s[0] : pad, t001 = z0in && y0in && x1in ? s[1] : pad;
            const float t010 = z0in && y1in && x0in ? s[vd.W] : pad, t011 = z0in && y1in && x1in ? s[vd.W + 1] : pad;
            const float t100 = z1in && y0in && x0in ? s[HW] : pad, t101 = z1in && y0in && x1in ? s[HW + 1] : pad;
            const float t110 = z1in && y1in && x0in ? s[HW + vd.W] : pad, t111 = z1in && y1in && x1in ? s[HW + vd.W + 1] : pad;
            const float v00 = t000 + wx * (t001 - t000), v01 = t010 + wx * (t011 - t010);
            const float v10 = t100 + wx * (t101 - t100), v11 = t110 + wx * (t111 - t110);
            const float v0 = v00 + wy * (v01 - v00), v1 = v10 + wy * (v11 - v10);
            const float v = v0 + wz * (v1 - v0);
            DT<TO>::st(out_img + ((long long)b * C + c) * R3 + orow + x, (v + row.shift) * row.scale);
        }
        const int nz = affine_index(floor(cz + 0.5), -1.0, vd.D), ny = affine_index(floor(cy + 0.5), -1.0, vd.H);
        const int nx = affine_index(floor(cx + 0.5), -1.0, vd.W);
        const bool in = vd.lab && nz >= 0 && nz < vd.D && ny >= 0 && ny < vd.H && nx >= 0 && nx < vd.W;
        out_lab[(long long)b * R3 + orow + x] = in ? (float)vd.lab[(long long)nz * HW + (long long)ny * vd.W + nx] : 0.0f;
    }
}

inline bool dims_ok(int C, int D, int H, int W) { return C >= 1 && D >= 1 && H >= 1 && W >= 1 && D <= 65535 && H <= 65535; }
inline dim3 row_grid(int D, int H, int W) { return dim3((unsigned)ceil_div(W, 256), (unsigned)H, (unsigned)D); }

}  // namespace

extern "C" {

int msseg_intensity_prep(const void* src, int src_dtype, int C, int D, int H, int W, int mode, float a_min, float a_range,
                         int normalize, float subtrahend, float divisor, float* dst, int* box6, msseg_stream_t stream) {
    if (!src || !dst || !box6 || !dims_ok(C, D, H, W) || mode < 0 || mode > 2 || (src_dtype != 0 && src_dtype != 1))
        MSSEG_FAIL(MSSEG_EINVAL, "intensity_prep: bad args (src fp32 = 0 / int16 = 1, mode 0..2, D, H <= 65535)");
    if (mode != 0 && a_range == 0.0f) MSSEG_FAIL(MSSEG_EINVAL, "intensity_prep: a_min == a_max");
    if (normalize && divisor == 0.0f) MSSEG_FAIL(MSSEG_EINVAL, "intensity_prep: zero divisor");
    hipLaunchKernelGGL(box_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, box6, D, H, W);
    if (src_dtype == 0)
        hipLaunchKernelGGL(intensity_prep_kernel<float>, row_grid(D, H, W), dim3(256), 0, (hipStream_t)stream,
                           (const float*)src, C, D, H, W, mode, a_min, a_range, normalize, subtrahend, divisor, dst, box6);
    else
        hipLaunchKernelGGL(intensity_prep_kernel<short>, row_grid(D, H, W), dim3(256), 0, (hipStream_t)stream,
                           (const short*)src, C, D, H, W, mode, a_min, a_range, normalize, subtrahend, divisor, dst, box6);
    MSSEG_CHECK_LAUNCH("intensity_prep");
    return MSSEG_OK;
}

int msseg_resample_spacing(const void* src, int is_label, int C, int SD, int SH, int SW, void* dst, int TD, int TH, int TW,
                           double rz, double ry, double rx, msseg_stream_t stream) {
    if (!src || !dst || !dims_ok(C, SD, SH, SW) || !dims_ok(C, TD, TH, TW) || !(rz > 0.0) || !(ry > 0.0) || !(rx > 0.0))
        MSSEG_FAIL(MSSEG_EINVAL, "resample_spacing: bad args");
    if (is_label)
        hipLaunchKernelGGL(resample_spacing_kernel<true>, row_grid(TD, TH, TW), dim3(256), 0, (hipStream_t)stream, src, C, SD,
                           SH, SW, dst, TD, TH, TW, rz, ry, rx);
    else
        hipLaunchKernelGGL(resample_spacing_kernel<false>, row_grid(TD, TH, TW), dim3(256), 0, (hipStream_t)stream, src, C, SD,
                           SH, SW, dst, TD, TH, TW, rz, ry, rx);
    MSSEG_CHECK_LAUNCH("resample_spacing");
    return MSSEG_OK;
}

int msseg_crop_pad_copy(const void* src, int elem_bytes, int C, int SD, int SH, int SW, const int* box6, void* dst, int TD,
                        int TH, int TW, const int* pad_before3, float pad_f32, int pad_u8, msseg_stream_t stream) {
    if (!src || !dst || !box6 || !pad_before3 || !dims_ok(C, SD, SH, SW) || !dims_ok(C, TD, TH, TW) ||
        (elem_bytes != 4 && elem_bytes != 1))
        MSSEG_FAIL(MSSEG_EINVAL, "crop_pad_copy: bad args (elem_bytes 4 = fp32, 1 = uint8)");
    const int z0 = box6[0], y0 = box6[1], x0 = box6[2], bd = box6[3] - z0, bh = box6[4] - y0, bw = box6[5] - x0;
    const int pz = pad_before3[0], py = pad_before3[1], px = pad_before3[2];
    if (z0 < 0 || y0 < 0 || x0 < 0 || bd < 1 || bh < 1 || bw < 1 || box6[3] > SD || box6[4] > SH || box6[5] > SW ||
        pz < 0 || py < 0 || px < 0 || pz + bd > TD || py + bh > TH || px + bw > TW)
        MSSEG_FAIL(MSSEG_EINVAL, "crop_pad_copy: box [%d:%d, %d:%d, %d:%d] of %dx%dx%d does not fit %dx%dx%d at pad (%d, %d, %d)",
                   z0, box6[3], y0, box6[4], x0, box6[5], SD, SH, SW, TD, TH, TW, pz, py, px);
    if (elem_bytes == 4)
        hipLaunchKernelGGL(crop_pad_copy_kernel<float>, row_grid(TD, TH, TW), dim3(256), 0, (hipStream_t)stream,
                           (const float*)src, C, SD, SH, SW, z0, y0, x0, bd, bh, bw, (float*)dst, TD, TH, TW, pz, py, px, pad_f32);
    else
        hipLaunchKernelGGL(crop_pad_copy_kernel<unsigned char>, row_grid(TD, TH, TW), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned char*)src, C, SD, SH, SW, z0, y0, x0, bd, bh, bw, (unsigned char*)dst, TD, TH, TW, pz,
                           py, px, (unsigned char)pad_u8);
    MSSEG_CHECK_LAUNCH("crop_pad_copy");
    return MSSEG_OK;
}

int msseg_slab_counts(const float* img0, const uint8_t* lab, int D, int H, int W, float threshold, int bg_rule, int* counts,
                      msseg_stream_t stream) {
    if (!img0 || !lab || !counts || D < 1 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL || bg_rule < 0 || bg_rule > 1)
        MSSEG_FAIL(MSSEG_EINVAL, "slab_counts: bad args");
    hipLaunchKernelGGL(slab_counts_kernel, dim3(D), dim3(256), 0, (hipStream_t)stream, img0, lab, H * W, threshold, bg_rule,
                       counts);
    MSSEG_CHECK_LAUNCH("slab_counts");
    return MSSEG_OK;
}

int msseg_pick_voxels(const void* volumes, int nvol, const void* rows, int nrows, int R, float threshold, int bg_rule, int* out,
                      msseg_stream_t stream) {
    if (!volumes || !rows || !out || nvol < 1 || nrows < 1 || R < 1 || bg_rule < 0 || bg_rule > 1)
        MSSEG_FAIL(MSSEG_EINVAL, "pick_voxels: bad args");
    hipLaunchKernelGGL(pick_voxels_kernel, dim3(nrows), dim3(256), 0, (hipStream_t)stream, (const VolDesc*)volumes, nvol,
                       (const PickRow*)rows, R, threshold, bg_rule, out);
    MSSEG_CHECK_LAUNCH("pick_voxels");
    return MSSEG_OK;
}

int msseg_aug_crop_multi(const void* volumes, int nvol, const void* rows, const int* picks, int npatch, int C, void* out_img,
                         int out_dtype, float* out_lab, int R, msseg_stream_t stream) {
    if (!volumes || !rows || !picks || !out_img || !out_lab || nvol < 1 || C < 1 || npatch < 1 || npatch > 65535 || R < 1 ||
        R > 65535)
        MSSEG_FAIL(MSSEG_EINVAL, "aug_crop_multi: bad args");
    const int nruns = ceil_div(R, 4);
    const int bx = nruns < 256 ? nruns : 256, by = 256 / bx;
    dim3 block(bx, by), grid((unsigned)ceil_div(R, by), (unsigned)R, (unsigned)npatch);
    const bool known = for_dtype(out_dtype, [&](auto t) {
        using TO = typename decltype(t)::type;
        hipLaunchKernelGGL(aug_crop_multi_kernel<TO>, grid, block, 0, (hipStream_t)stream, (const VolDesc*)volumes, nvol,
                           (const PickRow*)rows, picks, (TO*)out_img, out_lab, C, R);
    });
    if (!known) MSSEG_FAIL(MSSEG_EINVAL, "aug_crop_multi: bad dtype");
    MSSEG_CHECK_LAUNCH("aug_crop_multi");
    return MSSEG_OK;
}

int msseg_aug_crop_affine(const void* volumes, int nvol, const void* rows, const int* picks, const double* mats, int npatch,
                          int C, void* out_img, int out_dtype, float* out_lab, int R, float pad_value, msseg_stream_t stream) {
    if (!volumes || !rows || !picks || !mats || !out_img || !out_lab || nvol < 1 || C < 1 || npatch < 1 || npatch > 65535 ||
        R < 1 || R > 65535)
        MSSEG_FAIL(MSSEG_EINVAL, "aug_crop_affine: bad args");
    dim3 block(32, 8), grid((unsigned)ceil_div(R, 8), (unsigned)R, (unsigned)npatch);
    const bool known = for_dtype(out_dtype, [&](auto t) {
        using TO = typename decltype(t)::type;
        hipLaunchKernelGGL(aug_crop_affine_kernel<TO>, grid, block, 0, (hipStream_t)stream, (const VolDesc*)volumes, nvol,
                           (const PickRow*)rows, picks, mats, (TO*)out_img, out_lab, C, R, pad_value);
    });
    if (!known) MSSEG_FAIL(MSSEG_EINVAL, "aug_crop_affine: bad dtype");
    MSSEG_CHECK_LAUNCH("aug_crop_affine");
    return MSSEG_OK;
}

}  // extern "C"
