// Class-ratio crop centres on the device data path (RandCropByLabelClassesd, data/dataset_builder.py:88-136 of the
// reference; MONAI's map_classes_to_indices / generate_label_classes_crop_centers for the candidate sets).
//
// A voxel v is a candidate of class c < K iff image_ok(img0(v)) and some voxel u with lab(u) == c lies within L1 distance N
// of v (N = 0: lab(v) == c).  Labels >= K belong to no class.
//
//   class_candidate_mask  N > 0, once per cached volume: uint16 mask whose bit c is that predicate, for the classes of a bit
//                         set.  Per class three capped chamfer sweeps over one byte per voxel of scratch (distance to the
//                         class along x, then + y, then + z, capped at N + 1); the last sweep folds in image_ok and ORs the bit.
//   class_slab_counts     counts[z][c] from (img0, lab) or from the mask; one block per slice, integer counting
//   class_pick_voxels     pick_voxels with the per-class predicates: mode 16 + c is the rank-th candidate of class c of the
//                         slice; modes 0 / 1 / 2 as msseg_pick_voxels (one scan, pick_scan.h)
//
// Semantics: the numpy / scipy restatement in tests/class_crop_ref.py.  Geometry: lanes run along x everywhere.
#include "common.h"
#include "pick_scan.h"

namespace {

using pick::VolDesc;
using pick::PickRow;
using pick::bg_image_ok;

constexpr int MAX_CLASSES = 16;
constexpr int PICK_CLASS0 = 16;                                            // MSSEG_PICK_CLASS0

// x sweep, one wave per (z, y) row, 4 rows per block.  The row is walked in chunks of 64 voxels; a ballot of `lab == c`
// gives every lane the nearest class voxel of its chunk on either side (clz / ctz of the masked ballot), the nearest one of
// the chunks already walked is carried in a wave-uniform register.  Forward pass: distance to the left; backward pass: the
// minimum with the distance to the right.  Every lane re-reads only bytes it wrote itself.  dist: uint8 [D][H][W].
__global__ __launch_bounds__(256) void dilate_x_kernel(const unsigned char* __restrict__ lab, long long rows, int W, int c,
                                                       int cap, unsigned char* __restrict__ dist) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                                 // uniform over the wave
    const int lane = threadIdx.x & 63;
    const unsigned char* l = lab + r * W;
    unsigned char* d = dist + r * W;
    const int nchunk = (W + 63) / 64;
    int last = -1;                                                         // x of the nearest class voxel of earlier chunks
    for (int k = 0; k < nchunk; ++k) {
        const int x = k * 64 + lane;
        const bool is = x < W && l[x] == c;
        const unsigned long long m = __ballot(is);
        const unsigned long long left = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const int pos = left ? k * 64 + 63 - __builtin_clzll(left) : last;
        const int v = pos >= 0 && x - pos < cap ? x - pos : cap;
        if (x < W) d[x] = (unsigned char)v;
        if (m) last = k * 64 + 63 - __builtin_clzll(m);
    }
    int next = -1;                                                         // the same from the right
    for (int k = nchunk - 1; k >= 0; --k) {
        const int x = k * 64 + lane;
        const int cur = x < W ? (int)d[x] : cap;
        const unsigned long long m = __ballot(cur == 0);
        const unsigned long long right = m >> lane;
        const int pos = right ? x + __builtin_ctzll(right) : next;
        const int v = pos >= 0 && pos - x < cur ? pos - x : cur;
        if (x < W) d[x] = (unsigned char)v;
        if (m) next = k * 64 + __builtin_ctzll(m);
    }
}

// y sweep in place: one thread per (z, x) column, consecutive lanes on consecutive x.  grid: (x blocks, D)
__global__ __launch_bounds__(256) void dilate_y_kernel(unsigned char* __restrict__ dist, int H, int W, int cap) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    unsigned char* d = dist + (long long)blockIdx.y * H * W + x;
    int run = cap;
    for (int y = 0; y < H; ++y) {
        const int v = d[(long long)y * W];
        run = run + 1 < cap ? run + 1 : cap;
        run = v < run ? v : run;
        d[(long long)y * W] = (unsigned char)run;
    }
    run = cap;
    for (int y = H - 1; y >= 0; --y) {
        const int v = d[(long long)y * W];
        run = run + 1 < cap ? run + 1 : cap;
        run = v < run ? v : run;
        d[(long long)y * W] = (unsigned char)run;
    }
}

// z sweep: one thread per in-slice voxel i, consecutive lanes on consecutive i.  The forward pass writes the scratch; the
// backward pass knows the final distance and writes no scratch: within N and image_ok -> bit c of the mask.
__global__ __launch_bounds__(256) void dilate_z_mask_kernel(unsigned char* __restrict__ dist, const float* __restrict__ img0,
                                                            int D, long long HW, int cap, float thr, int rule, int c,
                                                            unsigned short* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    int run = cap;
    for (int z = 0; z < D; ++z) {
        const int v = dist[z * HW + i];
        run = run + 1 < cap ? run + 1 : cap;
        run = v < run ? v : run;
        dist[z * HW + i] = (unsigned char)run;
    }
    run = cap;
    const unsigned short bit = (unsigned short)(1u << c);
    for (int z = D - 1; z >= 0; --z) {
        const int v = dist[z * HW + i];
        run = run + 1 < cap ? run + 1 : cap;
        run = v < run ? v : run;
        if (run < cap && bg_image_ok(img0[z * HW + i], thr, rule)) mask[z * HW + i] |= bit;
    }
}

// the classes of one voxel as a bit set: from the mask, or bit lab of (img0, lab) under the image rule
struct VoxelBits {
    const unsigned short* mask; const unsigned char* lab; const float* img; float thr; int rule, K;
    MSSEG_DEVFN unsigned operator()(long long i) const {
        if (mask) return mask[i];
        const unsigned l = lab[i];
        return l < (unsigned)K && bg_image_ok(img[i], thr, rule) ? 1u << l : 0u;
    }
};

// one block per z-slice; counts[z][c] = number of candidates of class c in the slice.  16 counters per thread in registers
// (the loop over c is unrolled; bits >= K are never set), summed over the wave by shuffles and over the 4 waves in LDS.
__global__ __launch_bounds__(256) void class_slab_counts_kernel(VoxelBits bits, int HW, int K, int* __restrict__ counts) {
    __shared__ int part[4][MAX_CLASSES];
    const long long base = (long long)blockIdx.x * HW;
    int n[MAX_CLASSES];
#pragma unroll
    for (int c = 0; c < MAX_CLASSES; ++c) n[c] = 0;
    for (int i = threadIdx.x; i < HW; i += 256) {
        const unsigned b = bits(base + i);
#pragma unroll
        for (int c = 0; c < MAX_CLASSES; ++c) n[c] += (b >> c) & 1u;
    }
#pragma unroll
    for (int c = 0; c < MAX_CLASSES; ++c) {
        int v = n[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < K)
        counts[(long long)blockIdx.x * K + threadIdx.x] =
            part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// candidates of class c of one slice, N = 0: the label itself under the image rule
struct ClassPred {
    const unsigned char* lab; const float* img; float thr; int rule, c;
    MSSEG_DEVFN bool operator()(int i) const { return lab[i] == c && bg_image_ok(img[i], thr, rule); }
};
// the same read from the candidate mask
struct MaskPred {
    const unsigned short* mask; int c;
    MSSEG_DEVFN bool operator()(int i) const { return (mask[i] >> c) & 1; }
};

// one block per row, as pick_voxels_kernel; masks: NULL or nvol pointers to the volumes' candidate masks (NULL entries: none)
__global__ __launch_bounds__(256) void class_pick_voxels_kernel(const VolDesc* __restrict__ vols,
                                                                const unsigned short* const* __restrict__ masks, int nvol,
                                                                const PickRow* __restrict__ rows, int R, float thr, int rule,
                                                                int* __restrict__ out) {
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
    const long long off = (long long)z * HW;
    const int c = row.mode - PICK_CLASS0;
    int hit = -1;                                                           // a mode that names nothing: no candidate
    if (row.mode == 2) {
        hit = row.rank < 0 ? 0 : (row.rank >= HW ? HW - 1 : row.rank);      // explicit voxel of the slice
    } else if (row.mode == 0 || row.mode == 1) {
        const pick::FgBgPred pred{vd.lab + off, vd.img + off, thr, rule, row.mode == 1};
        hit = pick::scan_slice(HW, row.rank, pred, scan, &found);
    } else if (c >= 0 && c < MAX_CLASSES) {
        const unsigned short* mask = masks ? masks[row.vol] : nullptr;
        if (mask) {
            const MaskPred pred{mask + off, c};
            hit = pick::scan_slice(HW, row.rank, pred, scan, &found);
        } else {
            const ClassPred pred{vd.lab + off, vd.img + off, thr, rule, c};
            hit = pick::scan_slice(HW, row.rank, pred, scan, &found);
        }
    }
    if (threadIdx.x == 0) pick::write_pick(o, vd, z, hit, R);
}

inline bool vol_ok(int D, int H, int W) { return D >= 1 && H >= 1 && W >= 1 && D <= 65535 && (long long)H * W <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int msseg_class_candidate_mask(const float* img0, const uint8_t* lab, int D, int H, int W, float threshold, int bg_rule,
                               unsigned class_bits, int N, uint8_t* scratch, uint16_t* mask, msseg_stream_t stream) {
    if (!img0 || !lab || !scratch || !mask || !vol_ok(D, H, W) || bg_rule < 0 || bg_rule > 1)
        MSSEG_FAIL(MSSEG_EINVAL, "class_candidate_mask: bad args");
    if (N < 0 || N > 254) MSSEG_FAIL(MSSEG_EINVAL, "class_candidate_mask: dilation %d outside 0..254 (distances are bytes)", N);
    if (class_bits >> MAX_CLASSES) MSSEG_FAIL(MSSEG_EINVAL, "class_candidate_mask: classes 0..15 only");
    const long long HW = (long long)H * W, rows = (long long)D * H;
    if (ceil_div_ll(rows, 4) > 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "class_candidate_mask: volume too large");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(mask, 0, (size_t)D * HW * sizeof(uint16_t), s) != hipSuccess)
        MSSEG_FAIL(MSSEG_ELAUNCH, "class_candidate_mask: memset failed");
    const int cap = N + 1;
    for (int c = 0; c < MAX_CLASSES; ++c) {
        if (!((class_bits >> c) & 1u)) continue;
        hipLaunchKernelGGL(dilate_x_kernel, dim3((unsigned)ceil_div_ll(rows, 4)), dim3(256), 0, s, lab, rows, W, c, cap, scratch);
        hipLaunchKernelGGL(dilate_y_kernel, dim3((unsigned)ceil_div(W, 256), (unsigned)D), dim3(256), 0, s, scratch, H, W, cap);
        hipLaunchKernelGGL(dilate_z_mask_kernel, dim3((unsigned)ceil_div_ll(HW, 256)), dim3(256), 0, s, scratch, img0, D, HW, cap,
                           threshold, bg_rule, c, mask);
    }
    MSSEG_CHECK_LAUNCH("class_candidate_mask");
    return MSSEG_OK;
}

int msseg_class_slab_counts(const float* img0, const uint8_t* lab, const uint16_t* mask, int D, int H, int W, int K,
                            float threshold, int bg_rule, int* counts, msseg_stream_t stream) {
    if (!counts || !vol_ok(D, H, W) || K < 1 || K > MAX_CLASSES || bg_rule < 0 || bg_rule > 1 || (!mask && (!img0 || !lab)))
        MSSEG_FAIL(MSSEG_EINVAL, "class_slab_counts: bad args (1 <= K <= 16; a mask, or img0 and lab)");
    const VoxelBits bits{mask, lab, img0, threshold, bg_rule, K};
    hipLaunchKernelGGL(class_slab_counts_kernel, dim3(D), dim3(256), 0, (hipStream_t)stream, bits, H * W, K, counts);
    MSSEG_CHECK_LAUNCH("class_slab_counts");
    return MSSEG_OK;
}

int msseg_class_pick_voxels(const void* volumes, const void* masks, int nvol, const void* rows, int nrows, int R,
                            float threshold, int bg_rule, int* out, msseg_stream_t stream) {
    if (!volumes || !rows || !out || nvol < 1 || nrows < 1 || R < 1 || bg_rule < 0 || bg_rule > 1)
        MSSEG_FAIL(MSSEG_EINVAL, "class_pick_voxels: bad args");
    hipLaunchKernelGGL(class_pick_voxels_kernel, dim3(nrows), dim3(256), 0, (hipStream_t)stream, (const VolDesc*)volumes,
                       (const unsigned short* const*)masks, nvol, (const PickRow*)rows, R, threshold, bg_rule, out);
    MSSEG_CHECK_LAUNCH("class_pick_voxels");
    return MSSEG_OK;
}

}  // extern "C"
