// ConvTranspose3d k = s = S (S = 2: deconv_k2s2_gen.hip, S = 4: deconv_k4s4.hip), bf16: the kernel parameters of both files and
// the forward kernel they share.  Eligibility, instantiation choice and grid caps differ per stride on purpose and stay with
// the callers.
#pragma once
#include "common.h"

struct DeconvParams {
    const void* x; long long ldx;      // coarse [N, D, H, W, Cin]    (forward input / backward output dx)
    const void* wp;                    // packed image (forward: M = S^3 * Cout, K = Cin; backward: M = Cin, K = S^3 * Cout)
    const float* bias;
    void* y; long long ldy;            // fine [N, S*D, S*H, S*W, Cout] (forward output / backward input dy)
    int N, D, H, W, Cin, Cout;
    int cb, nkb;                       // cout block width and k-blocks of the image
    float* part;                       // k2 backward: fp32 [Cin / 4][N*D*H*W][4] instead of bf16 dx
};

constexpr int DECONV_THREADS = 256;

// A wave takes 16 coarse voxels along W; grid.y slices the output by (child group, cout slice).  A child group is all S children
// of one fine row (a, b) -- those of the 16 voxels form ONE run of 16 * S fine voxels -- or a single child (every S-th fine
// voxel).  The results are transposed through a wave-private LDS tile into 16-byte stores.  The B operand comes straight from
// the channels-last rows, the slice's weights live in registers.
template <int S, int KS, int NH, int CH>   // KS = ceil(Cin / 32) k-steps, NH cout tiles per slice, CH children per slice (S or 1)
__global__ __launch_bounds__(DECONV_THREADS, 2) void deconv_sliced_fwd_kernel(const DeconvParams p) {
    static_assert(CH == S || CH == 1, "a slice is a whole fine row or one child");
    constexpr int CS = NH * 16;                         // channels of a slice
    constexpr int RSB = CS * 2 + 16;                    // LDS bytes per fine voxel (16-byte pad: fewer write conflicts)
    constexpr int FV = 16 * CH;                         // fine voxels of a segment that this slice writes
    constexpr int TILE_B = FV * RSB;
    constexpr int CPV = CS * 2 / 16;                    // 16-byte chunks per fine voxel
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * TILE_B];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    unsigned char* tile = lds + wave * TILE_B;
    const bf16_t* __restrict__ xg = (const bf16_t*)p.x;
    const int nsl = p.Cout / CS;
    const int cg = blockIdx.y / nsl, js = blockIdx.y - cg * nsl;
    const int abc0 = cg * CH;                           // first child of the slice, abc = (a * S + b) * S + c
    const int cbase = js * CS;
    bf16_t* __restrict__ yg = (bf16_t*)p.y + cbase;

    u32x4_t af[CH][NH][KS];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < NH; ++j)
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                const int m0 = (abc0 + c) * p.Cout + cbase + j * 16;
                const int blk = m0 / p.cb, row = m0 - blk * p.cb + r;
                af[c][j][k] = ldg16((const unsigned char*)p.wp + wimg_frag_off(blk, KS, k, q, p.cb, row));
            }
    f32x4_t bv[NH];
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        bv[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (p.bias) bv[j] = *(const f32x4_t*)(p.bias + cbase + j * 16 + q * 4);
    }
    bool kok[KS];                                       // this lane's chunk of k-step k lies inside the row
#pragma unroll
    for (int k = 0; k < KS; ++k) kok[k] = k * 32 + q * 8 < p.Cin;

    const int GW = (p.W + 15) >> 4;
    const long long groups = (long long)p.N * p.D * p.H * GW;
    const long long wstride = (long long)gridDim.x * 4;
    for (long long g = (long long)blockIdx.x * 4 + wave; g < groups; g += wstride) {
        const int gw = (int)(g % GW);
        long long t = g / GW;
        const int h = (int)(t % p.H); t /= p.H;
        const int d = (int)(t % p.D);
        const long long n = t / p.D;
        const int w0 = gw * 16, w = w0 + r;
        const bool valid = w < p.W;
        const long long cvox = ((n * p.D + d) * p.H + h) * p.W + w;
        u32x4_t bx[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k)
            bx[k] = (valid && kok[k]) ? ldg16(xg + cvox * p.ldx + k * 32 + q * 8) : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                f32x4_t acc = bv[j];
#pragma unroll
                for (int k = 0; k < KS; ++k) mma_chunk<bf16_t>(acc, af[c][j][k], bx[k]);
                const bf16x4_t o = {(bf16_t)acc[0], (bf16_t)acc[1], (bf16_t)acc[2], (bf16_t)acc[3]};
                *(bf16x4_t*)(tile + (CH * r + c) * RSB + (j * 16 + q * 4) * 2) = o;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private tile: LDS ops of one wave execute in order
        const int ncv = (p.W - w0) < 16 ? (p.W - w0) : 16;   // valid coarse voxels of this segment
        const long long frow = ((n * S * p.D + S * d + abc0 / (S * S)) * S * p.H + S * h + (abc0 / S) % S) * S * p.W + S * w0;
#pragma unroll
        for (int it = 0; it < (FV * CPV + 63) / 64; ++it) {
            const int ch = it * 64 + lane;
            const int fv = ch / CPV, part = ch - fv * CPV;
            if (ch < FV * CPV && fv < CH * ncv) {
                const u32x4_t v = *(const u32x4_t*)(tile + fv * RSB + part * 16);
                const long long fw = CH == S ? fv : S * fv + abc0 % S;
                *(u32x4_t*)(yg + (frow + fw) * p.ldy + part * 8) = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads are done before the next group's writes
    }
}
