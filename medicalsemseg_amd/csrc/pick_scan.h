// The crop-centre pick shared by dataprep.hip (fg / bg candidates) and class_crop.hip (per-class candidates): the volume and
// row tables, the image side of a candidate, the MONAI centre clamp, the counting scan of one slice under a predicate and
// the output row.  Device code only.
#pragma once
#include "common.h"

namespace pick {

struct VolDesc { const float* img; const unsigned char* lab; int C, D, H, W; };              // mirrors msseg_volume_desc
struct PickRow { int vol, mode, z, rank, flips, rotk; float shift, scale; };                   // mirrors msseg_pick_row

// the image side of a crop-centre candidate: rule 0 = above the threshold (the reference's image_threshold on a cache
// whose scale is monotone in the raw one), rule 1 = different from it (the non-zero mask of a z-scored cache, whose
// in-mask values have either sign)
MSSEG_DEVFN bool bg_image_ok(float v, float thr, int rule) { return rule ? v != thr : v > thr; }

// MONAI correct_crop_centers for one axis (oracle/augment.py): centre clamped so that the roi stays inside the image
MSSEG_DEVFN int clamp_center(int c, int r, int n) {
    const int lo = r / 2;
    int hi = n + 1 - r / 2;      // floor for even r, ceil for odd r of n + 1 - r / 2.0
    if (lo == hi) hi += 1;
    c = c < lo ? lo : c;
    c = c >= hi ? hi - 1 : c;
    return c;
}

// candidates of the fg / bg crop: label > 0, or label == 0 with the image rule
struct FgBgPred {
    const unsigned char* lab; const float* img; float thr; int rule; bool want_fg;
    MSSEG_DEVFN bool operator()(int i) const {
        const unsigned char l = lab[i];
        return want_fg ? (l > 0) : (l == 0 && bg_image_ok(img[i], thr, rule));
    }
};

// Counting scan of one slice of HW voxels in flat order, chunks of 256 threads x PICK_K voxels: the in-slice index of the
// rank-th voxel with pred(i), -1 when the slice has no more than `rank` of them.  Every thread of a 256-thread block calls
// it with the same arguments; `scan` (256 ints) and `found` are the block's shared memory.
constexpr int PICK_K = 8;
template <typename Pred>
MSSEG_DEVFN int scan_slice(int HW, int rank, const Pred& pred, int* scan, int* found) {
    if (threadIdx.x == 0) *found = -1;
    int running = 0;
    for (int base = 0; base < HW; base += 256 * PICK_K) {
        const int first = base + threadIdx.x * PICK_K;
        int n = 0;
#pragma unroll
        for (int j = 0; j < PICK_K; ++j) {
            const int i = first + j;
            if (i < HW) n += pred(i);
        }
        scan[threadIdx.x] = n;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {                              // inclusive prefix sum over the block
            const int v = threadIdx.x >= s ? scan[threadIdx.x - s] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        const int incl = scan[threadIdx.x], total = scan[255];
        const int want = rank - running;                                 // rank inside this chunk
        if (want >= 0 && want < total && want >= incl - n && want < incl) {
            int k = want - (incl - n);
            for (int j = 0; j < PICK_K; ++j) {
                const int i = first + j;
                if (i < HW && pred(i) && k-- == 0) { *found = i; break; }
            }
        }
        __syncthreads();
        if (want >= 0 && want < total) break;                            // uniform over the block
        running += total;
    }
    __syncthreads();
    return *found;
}

// out[8] = {centre z, y, x (clamped for the cubic roi R), crop start z, y, x, z, in-slice flat index or -1}
MSSEG_DEVFN void write_pick(int* o, const VolDesc& vd, int z, int hit, int R) {
    const int py = hit >= 0 ? hit / vd.W : 0, px = hit >= 0 ? hit % vd.W : 0;
    const int cz = clamp_center(z, R, vd.D), cy = clamp_center(py, R, vd.H), cx = clamp_center(px, R, vd.W);
    o[0] = cz; o[1] = cy; o[2] = cx;
    o[3] = cz - R / 2; o[4] = cy - R / 2; o[5] = cx - R / 2;
    o[6] = z; o[7] = hit;                                                // hit == -1: rank beyond the slice's count
}

}  // namespace pick
