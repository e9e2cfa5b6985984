// Prediction -> native grid: the inverse of data_device.preprocess_volume in one launch.
//
//   restore_native_u8   un-pad, un-crop, inverse Spacingd, un-flip / un-permute of a label map (nearest) or of the logits
//                       (trilinear + arg max, never forming [C][native]); one byte per voxel of the file's array comes out
//
// Per native voxel n and oriented axis k (native axis perm[k]): o = n[perm[k]], reversed when flip[k];
// s = min((double)o * scale[k], grid[k] - 1); m = s + offset[k]; q = floor(m + 0.5).  A q outside the model grid was cropped
// away as air: class 0.  Nearest: src[q].  Linear: taps floor(m) and floor(m) + 1 clamped into the model grid, fp32 lerps
// a + f * (b - a) along model axis 2, 1, 0 (resample_spacing_kernel's order), first strictly greatest channel
// (argmax_u8_kernel's rule).  One rounding per operation.
//
// Shape: a thread makes 4 consecutive voxels of native axis 2 and stores them as one dword; whatever depends on native
// axes 0 and 1 only is computed once per thread from the launch grid.  The kernel works in NATIVE axis order: the host folds
// the permutation into per-native-axis strides, so the gather itself does not know it; only the lerp order does (template
// parameter K2 = the model axis native axis 2 lands on).  Block footprint:
//   K2 == 2  native axis 2 is the model's fastest axis: 64 quads x 4 rows of native axis 1; loads and stores are runs, a wave
//            stores 256 contiguous bytes.
//   K2 != 2  the loads are strided by a model row or slice per native voxel.  The block is 4 quads x 64 rows, the rows walking
//            the native axis that IS the model's fastest one, so a wave is 4 quads x 16 rows: one load instruction touches 4
//            source lines with 16 consecutive elements each, the 16 lines a block touches are each used by 64 neighbouring
//            rows (256 B of fp32 logits, 64 B of labels), and a wave stores 16 segments of 16 contiguous bytes which the
//            blocks to its sides complete to full lines in L2.  What a wave's LOADS touch decides: there are 8 C of them
//            per voxel and one store per four voxels (the block shapes measured: profiles/README.md).
#include "common.h"

#include <cmath>

namespace {

// the descriptor in native axis order, as the kernel takes it (by value)
struct RestoreArgs {
    int native[3];        // file array shape
    int flip[3];          // native axis a runs backwards
    int grid[3];          // length of its oriented axis after the spacing resample
    int offset[3];        // pad_before - box_lo of that axis
    int model[3];         // length of that axis on the model grid
    int kax[3];           // the model axis native axis a lands on
    long long stride[3];  // element stride of that model axis in src
    double scale[3];
    int row_axis;         // native axis threadIdx.y walks (1, or 0 when native axis 0 is the model's fastest)
};

struct AxisPos { int q; bool in; int lo, hi; float f; };

// one axis of one voxel: the nearest index (and whether it is on the model grid), the two clamped taps and the fraction
MSSEG_DEVFN AxisPos axis_pos(const RestoreArgs& A, int a, int o) {
#pragma clang fp contract(off)
    if (A.flip[a]) o = A.native[a] - 1 - o;
    double s = (double)o * A.scale[a];
    const double last = (double)(A.grid[a] - 1);
    if (s > last) s = last;                                   // resample_shape rounds: the tail may overshoot by half a voxel
    const double m = s + (double)A.offset[a];
    const double q = floor(m + 0.5), i0 = floor(m), top = (double)(A.model[a] - 1);
    AxisPos p;
    p.in = q >= 0.0 && q <= top;
    p.q = (int)fmin(fmax(q, 0.0), top);
    p.lo = (int)fmin(fmax(i0, 0.0), top);
    p.hi = (int)fmin(fmax(i0 + 1.0, 0.0), top);
    p.f = (float)(m - i0);
    return p;
}

MSSEG_DEVFN void store_quad(unsigned char* dst, long long o, int n, const unsigned char* v) {
    if (n == 4 && ((uintptr_t)(dst + o) & 3) == 0) {
        *(uint32_t*)(dst + o) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
        for (int e = 0; e < n; ++e) dst[o + e] = v[e];
    }
}

// the thread's place: quad of native axis 2 from x, the row axis from y, the remaining axis from z
#define RESTORE_PLACE()                                                                                     \
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;                                            \
    const int r = blockIdx.y * blockDim.y + threadIdx.y, t = blockIdx.z;                                   \
    const int n0 = A.row_axis == 0 ? r : t, n1 = A.row_axis == 0 ? t : r;                                  \
    if (x4 >= A.native[2] || n0 >= A.native[0] || n1 >= A.native[1]) return;                               \
    const int n = A.native[2] - x4 < 4 ? A.native[2] - x4 : 4;                                             \
    const long long orow = ((long long)n0 * A.native[1] + n1) * A.native[2] + x4

__global__ __launch_bounds__(256) void restore_nearest_kernel(const unsigned char* __restrict__ src, RestoreArgs A,
                                                              unsigned char* __restrict__ dst) {
    RESTORE_PLACE();
    const AxisPos p0 = axis_pos(A, 0, n0), p1 = axis_pos(A, 1, n1);
    const long long base = (long long)p0.q * A.stride[0] + (long long)p1.q * A.stride[1];
    const bool in01 = p0.in && p1.in;
    unsigned char v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < n) {
            const AxisPos p2 = axis_pos(A, 2, x4 + e);
            if (in01 && p2.in) v[e] = src[base + (long long)p2.q * A.stride[2]];
        }
    }
    store_quad(dst, orow, n, v);
}

// K2: the model axis of native axis 2.  KA < KB are the other two model axes; their positions are the thread's.
// The thread's four voxels while it computes, xe[e]:
//   K2 != 2  the quad it stores, x4 + e: the loads are strided along native axis 2 whatever the thread takes.
//   K2 == 2  xb + 64 e + lane (block (64, 4): a wave is one row, xb the block's first voxel): the lanes of one load
//            instruction read consecutive floats (two cache lines, against eight when every lane walks its own quad).  The
//            wave's 256 results are then regrouped with lane shuffles, so that lane j still stores voxels 4j .. 4j + 3.
template <int K2>
__global__ __launch_bounds__(256) void restore_linear_kernel(const float* __restrict__ src, int C, long long MV, RestoreArgs A,
                                                             unsigned char* __restrict__ dst) {
#pragma clang fp contract(off)   // every lerp is a subtraction, a product and a sum, each rounded
    const int r = blockIdx.y * blockDim.y + threadIdx.y, t = blockIdx.z;
    const int n0 = A.row_axis == 0 ? r : t, n1 = A.row_axis == 0 ? t : r;
    if (n0 >= A.native[0] || n1 >= A.native[1]) return;       // K2 == 2: uniform over the wave, the shuffles see all lanes
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (K2 != 2 && x4 >= A.native[2]) return;
    constexpr int KA = K2 == 0 ? 1 : 0;                        // KB = K2 == 2 ? 1 : 2
    const AxisPos p0 = axis_pos(A, 0, n0), p1 = axis_pos(A, 1, n1);
    const bool a_is_0 = A.kax[0] == KA;                       // native axis 0 is model axis KA (else native axis 1 is)
    const AxisPos pa = a_is_0 ? p0 : p1, pb = a_is_0 ? p1 : p0;
    const long long sa = a_is_0 ? A.stride[0] : A.stride[1], sb = a_is_0 ? A.stride[1] : A.stride[0];
    const long long alo = pa.lo * sa, ahi = pa.hi * sa, blo = pb.lo * sb, bhi = pb.hi * sb;
    const bool in01 = p0.in && p1.in;
    long long vlo[4], vhi[4];
    float vf[4];
    bool in[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int xe = K2 == 2 ? blockIdx.x * 256 + 64 * e + (int)threadIdx.x : x4 + e;
        const AxisPos p2 = axis_pos(A, 2, xe < A.native[2] ? xe : 0);       // a voxel past the row: computed, never stored
        vlo[e] = p2.lo * A.stride[2]; vhi[e] = p2.hi * A.stride[2]; vf[e] = p2.f; in[e] = in01 && p2.in;
    }
    float best[4];
    unsigned char v[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
        const float* s = src + (long long)c * MV;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // offsets and fractions in model axis order (0, 1, 2)
            const long long l0 = K2 == 0 ? vlo[e] : alo, h0 = K2 == 0 ? vhi[e] : ahi;
            const long long l1 = K2 == 1 ? vlo[e] : (K2 == 0 ? alo : blo), h1 = K2 == 1 ? vhi[e] : (K2 == 0 ? ahi : bhi);
            const long long l2 = K2 == 2 ? vlo[e] : blo, h2 = K2 == 2 ? vhi[e] : bhi;
            const float f0 = K2 == 0 ? vf[e] : pa.f, f1 = K2 == 1 ? vf[e] : (K2 == 0 ? pa.f : pb.f);
            const float f2 = K2 == 2 ? vf[e] : pb.f;
            const float t000 = s[l0 + l1 + l2], t001 = s[l0 + l1 + h2], t010 = s[l0 + h1 + l2], t011 = s[l0 + h1 + h2];
            const float t100 = s[h0 + l1 + l2], t101 = s[h0 + l1 + h2], t110 = s[h0 + h1 + l2], t111 = s[h0 + h1 + h2];
            const float v00 = t000 + f2 * (t001 - t000), v01 = t010 + f2 * (t011 - t010);
            const float v10 = t100 + f2 * (t101 - t100), v11 = t110 + f2 * (t111 - t110);
            const float v0 = v00 + f1 * (v01 - v00), v1 = v10 + f1 * (v11 - v10);
            const float val = v0 + f0 * (v1 - v0);
            if (c == 0) best[e] = val;
            else if (val > best[e]) { best[e] = val; v[e] = (unsigned char)c; }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (!in[e]) v[e] = 0;
    if (K2 == 2) {
        // voxel 4j + i of the wave's 256 sits in lane (4j + i) % 64, register (4j + i) / 64 = j / 16
        const int j = threadIdx.x;
        const int all = (int)v[0] | ((int)v[1] << 8) | ((int)v[2] << 16) | ((int)v[3] << 24);
        unsigned char o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (unsigned char)((unsigned)__shfl(all, (4 * j + i) & 63) >> (8 * (j >> 4)));
        v[0] = o[0]; v[1] = o[1]; v[2] = o[2]; v[3] = o[3];
        if (x4 >= A.native[2]) return;
    }
    const int n = A.native[2] - x4 < 4 ? A.native[2] - x4 : 4;
    store_quad(dst, ((long long)n0 * A.native[1] + n1) * A.native[2] + x4, n, v);
}

}  // namespace

extern "C" {

int msseg_restore_native_u8(const void* src, int src_is_logits, int C, const void* desc, uint8_t* dst, msseg_stream_t stream) {
    if (!src || !desc || !dst) MSSEG_FAIL(MSSEG_EINVAL, "restore_native_u8: null pointer");
    const msseg_restore_desc d = *(const msseg_restore_desc*)desc;
    int seen = 0;
    for (int k = 0; k < 3; ++k) {
        if (d.perm[k] < 0 || d.perm[k] > 2) MSSEG_FAIL(MSSEG_EINVAL, "restore_native_u8: perm[%d] = %d", k, d.perm[k]);
        seen |= 1 << d.perm[k];
        if (d.native[k] < 1 || d.grid[k] < 1 || d.model[k] < 1)
            MSSEG_FAIL(MSSEG_EINVAL, "restore_native_u8: axis %d has a dimension < 1 (native %d, grid %d, model %d)", k,
                       d.native[k], d.grid[k], d.model[k]);
        if (!std::isfinite(d.scale[k]) || !(d.scale[k] > 0.0))
            MSSEG_FAIL(MSSEG_EINVAL, "restore_native_u8: scale[%d] = %g is not a finite positive number", k, d.scale[k]);
    }
    if (seen != 7) MSSEG_FAIL(MSSEG_EINVAL, "restore_native_u8: perm (%d, %d, %d) is not a permutation", d.perm[0], d.perm[1], d.perm[2]);
    if (d.native[0] > 65535 || d.native[1] > 65535)
        MSSEG_FAIL(MSSEG_EINVAL, "restore_native_u8: native axes 0 and 1 hold at most 65535 voxels");
    if (src_is_logits && (C < 1 || C > 255)) MSSEG_FAIL(MSSEG_EINVAL, "restore_native_u8: C = %d outside 1..255", C);
    RestoreArgs A;
    const long long mstride[3] = {(long long)d.model[1] * d.model[2], (long long)d.model[2], 1};
    for (int k = 0; k < 3; ++k) {
        const int a = d.perm[k];
        A.native[a] = d.native[a];
        A.flip[a] = d.flip[k] != 0; A.grid[a] = d.grid[k]; A.offset[a] = d.offset[k]; A.model[a] = d.model[k];
        A.kax[a] = k; A.stride[a] = mstride[k]; A.scale[a] = d.scale[k];
    }
    const int k2 = A.kax[2];
    A.row_axis = d.perm[2] == 0 ? 0 : 1;
    const int bx = k2 == 2 ? 64 : 4, by = 256 / bx;
    const int rows = d.native[A.row_axis], other = d.native[1 - A.row_axis];
    dim3 block(bx, by), grid((unsigned)ceil_div(ceil_div(d.native[2], 4), bx), (unsigned)ceil_div(rows, by), (unsigned)other);
    if (!src_is_logits) {
        hipLaunchKernelGGL(restore_nearest_kernel, grid, block, 0, (hipStream_t)stream, (const unsigned char*)src, A, dst);
    } else {
        const long long MV = mstride[0] * d.model[0];
        if (k2 == 0)
            hipLaunchKernelGGL(restore_linear_kernel<0>, grid, block, 0, (hipStream_t)stream, (const float*)src, C, MV, A, dst);
        else if (k2 == 1)
            hipLaunchKernelGGL(restore_linear_kernel<1>, grid, block, 0, (hipStream_t)stream, (const float*)src, C, MV, A, dst);
        else
            hipLaunchKernelGGL(restore_linear_kernel<2>, grid, block, 0, (hipStream_t)stream, (const float*)src, C, MV, A, dst);
    }
    MSSEG_CHECK_LAUNCH("restore_native_u8");
    return MSSEG_OK;
}

}  // extern "C"
