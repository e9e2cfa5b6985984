// The x line scan that the distance passes of hausdorff.hip (voxel units) and surface_mm.hip (millimetres) both start from.
#pragma once
#include "common.h"

namespace {

constexpr int HD_INF16 = 0xFFFF;

struct HdBox { int z0, y0, x0, z1, y1, x1; };   // half-open

// pass x: one thread per (z, y) line of the box; gx[z][y][x] = distance along the line to the nearest surface voxel of
// class `cls` in `src` (0xFFFF: none on this line).  Box-local output layout [bz][by][bx].
__global__ __launch_bounds__(256) void hd_pass_x_kernel(const unsigned char* __restrict__ src, int cls, int H, int W,
                                                        HdBox b, unsigned short* __restrict__ gx) {
    const int by = b.y1 - b.y0, bx = b.x1 - b.x0, bz = b.z1 - b.z0;
    const long long lines = (long long)bz * by;
    for (long long l = blockIdx.x * 256LL + threadIdx.x; l < lines; l += (long long)gridDim.x * 256) {
        const int y = (int)(l % by), z = (int)(l / by);
        const unsigned char* row = src + ((long long)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0;
        unsigned short* out = gx + l * bx;
        int last = -HD_INF16;
        for (int x = 0; x < bx; ++x) {
            if (row[x] == cls) last = x;
            const int d = x - last;
            out[x] = (unsigned short)(d < HD_INF16 ? d : HD_INF16);
        }
        last = 2 * HD_INF16;
        for (int x = bx - 1; x >= 0; --x) {
            if (row[x] == cls) last = x;
            const int d = last - x;
            if (d < (int)out[x]) out[x] = (unsigned short)d;
        }
    }
}

}  // namespace
