// Region-based inference: sigmoid logits -> label map (threshold at 0, regions painted in their listed order), and the
// per-region overlap counts of two uint8 label maps.  The region table travels by value in the kernel arguments.
#include "common.h"

namespace {

struct region_values { uint8_t v[16]; };

// four consecutive voxels per thread where V and the pointers allow it (one 16-byte load per channel, one 4-byte store);
// the channel loop is unrolled to CMAX so that every row is requested before the first comparison
template <int CMAX>
__global__ __launch_bounds__(256) void region_decode_kernel(const float* __restrict__ logits, int C, long long V,
                                                            const region_values rv, uint8_t* __restrict__ out,
                                                            uint16_t* __restrict__ bits, int vec4) {
    const long long stride = (long long)gridDim.x * 256;
    auto paint = [&](unsigned b) {
        unsigned o = 0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if ((b >> c) & 1u) o = rv.v[c];
        return o;
    };
    if (vec4) {
        const long long Q = V >> 2;
        for (long long q = blockIdx.x * 256LL + threadIdx.x; q < Q; q += stride) {
            f32x4_t x[CMAX];
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                x[c] = c < C ? *(const f32x4_t*)(logits + (long long)c * V + 4 * q) : f32x4_t{0.f, 0.f, 0.f, 0.f};
            unsigned b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] |= (c < C && x[c][j] > 0.f) ? (1u << c) : 0u;   // NaN > 0 is false
            const unsigned o = paint(b[0]) | (paint(b[1]) << 8) | (paint(b[2]) << 16) | (paint(b[3]) << 24);
            *(uint32_t*)(out + 4 * q) = o;
            if (bits) *(u32x2_t*)(bits + 4 * q) = u32x2_t{b[0] | (b[1] << 16), b[2] | (b[3] << 16)};
        }
        return;
    }
    for (long long v = blockIdx.x * 256LL + threadIdx.x; v < V; v += stride) {
        float x[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) x[c] = c < C ? logits[(long long)c * V + v] : 0.f;
        unsigned b = 0u;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) b |= (c < C && x[c] > 0.f) ? (1u << c) : 0u;
        out[v] = (uint8_t)paint(b);
        if (bits) bits[v] = (uint16_t)b;
    }
}

// rows[block][c][0..2] = this block's (|P_c & T_c|, |P_c|, |T_c|) as unsigned counts
__global__ __launch_bounds__(256) void region_counts_kernel(const uint8_t* __restrict__ pred,
                                                            const uint8_t* __restrict__ label, long long V, int C,
                                                            const msseg_region_masks rm, unsigned* __restrict__ rows,
                                                            long long vox_per_block) {
    __shared__ unsigned red[4][48];
    const long long v0 = (long long)blockIdx.x * vox_per_block;
    long long v1 = v0 + vox_per_block;
    if (v1 > V) v1 = V;
    unsigned acc[16][3];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c][0] = acc[c][1] = acc[c][2] = 0u;
    for (long long v = v0 + threadIdx.x; v < v1; v += 256) {
        const unsigned p = pred[v], t = label[v];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const unsigned m = rm.mask[c];   // 0 past the last region
            const unsigned pb = p < 32u ? (m >> (p & 31u)) & 1u : 0u, tb = t < 32u ? (m >> (t & 31u)) & 1u : 0u;
            acc[c][0] += pb & tb;
            acc[c][1] += pb;
            acc[c][2] += tb;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < 16; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            unsigned s = acc[c][k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) red[wave][c * 3 + k] = s;
        }
    __syncthreads();
    if ((int)threadIdx.x < C * 3)
        rows[(long long)blockIdx.x * 48 + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// counts[c][k] = sum over the blocks' rows, in block order, in 64-bit integers
__global__ __launch_bounds__(64) void region_counts_finalize_kernel(const unsigned* __restrict__ rows, int nblk, int C,
                                                                    float* __restrict__ counts) {
    const int i = threadIdx.x;
    if (i >= C * 3) return;
    unsigned long long s = 0ull;
    for (int b = 0; b < nblk; ++b) s += rows[(long long)b * 48 + i];
    counts[i] = (float)s;
}

}  // namespace

extern "C" {

int msseg_region_decode_u8(const float* logits, int C, long long V, const uint8_t* values, uint8_t* out, uint16_t* bits,
                           msseg_stream_t stream) {
    if (C < 1 || C > 16) MSSEG_FAIL(MSSEG_EINVAL, "region_decode_u8: 1 <= C <= 16 regions (got %d)", C);
    if (!logits || !values || !out || V < 1) MSSEG_FAIL(MSSEG_EINVAL, "region_decode_u8: bad args");
    region_values rv = {};
    for (int c = 0; c < C; ++c) rv.v[c] = values[c];
    const int vec4 = (V % 4 == 0) && !(((uintptr_t)logits & 15) || ((uintptr_t)out & 3) || ((uintptr_t)bits & 7));
    const int grid = stream_grid(vec4 ? V / 4 : V, 256);
#define LAUNCH_DECODE(CM)                                                                                            \
    hipLaunchKernelGGL(region_decode_kernel<CM>, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, C, V, rv, out, \
                       bits, vec4)
    if (C <= 4) LAUNCH_DECODE(4);
    else if (C <= 8) LAUNCH_DECODE(8);
    else LAUNCH_DECODE(16);
#undef LAUNCH_DECODE
    MSSEG_CHECK_LAUNCH("region_decode_u8");
    return MSSEG_OK;
}

int msseg_region_counts_u8(const uint8_t* pred, const uint8_t* label, long long V, int C, const msseg_region_masks* masks,
                           float* counts, void* scratch, size_t scratch_bytes, msseg_stream_t stream) {
    if (C < 1 || C > 16) MSSEG_FAIL(MSSEG_EINVAL, "region_counts_u8: 1 <= C <= 16 regions (got %d)", C);
    if (!pred || !label || !masks || !counts || V < 1) MSSEG_FAIL(MSSEG_EINVAL, "region_counts_u8: bad args");
    const int rc = scratch_ok(scratch, scratch_bytes, "region_counts_u8");
    if (rc) return rc;
    msseg_region_masks rm = {};
    for (int c = 0; c < C; ++c) rm.mask[c] = masks->mask[c];
    // at most 1024 rows for the one-block second step; a block counts at most 2^22 voxels, far below what its unsigned
    // counts hold
    long long blocks = stream_grid(V, 256LL * 16);
    if (blocks > 1024) blocks = 1024;
    long long vpb = ceil_div_ll(V, blocks);
    if (vpb > (1LL << 22)) vpb = 1LL << 22;
    blocks = ceil_div_ll(V, vpb);
    if ((size_t)blocks * 48 * 4 > scratch_bytes - MSSEG_SCRATCH_HEADER_BYTES)
        MSSEG_FAIL(MSSEG_EINVAL, "region_counts_u8: %lld voxels are more than the scratch holds block rows for", V);
    unsigned* rows = (unsigned*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    hipLaunchKernelGGL(region_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred, label, V, C,
                       rm, rows, vpb);
    MSSEG_CHECK_LAUNCH("region_counts_u8");
    hipLaunchKernelGGL(region_counts_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, rows, (int)blocks, C,
                       counts);
    MSSEG_CHECK_LAUNCH("region_counts_finalize");
    return MSSEG_OK;
}

}  // extern "C"
