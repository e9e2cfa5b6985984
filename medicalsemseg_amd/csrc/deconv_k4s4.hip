// ConvTranspose3d k = s = 4 for gfx950: the last up block of Swin-UNETR with patch size 4 (hidden -> hidden, vol/4 -> vol).
//
//   y[n, 4d+a, 4h+b, 4w+c, co] = bias[co] + sum_ci x[n,d,h,w,ci] * W[ci,co,a,b,c]          64 children per coarse voxel
//
// Weight images are the ones of msseg_pack_weights (T = 1), as for k2 s2 with 8 -> 64:
//   forward / weight gradient   M = abc * Cout + co (abc = (a*4 + b)*4 + c), K = ci
//   input gradient              M = ci, K = abc * Cout + co
//
// bf16 fast path (Cin = Cout in {32, 48, 64, 96}; the forward takes a few more shapes), same scheme as deconv_k2s2_gen.hip:
//   forward   a wave takes 16 coarse voxels along W; grid.y slices the output by (fine row ab, cout slice).  The four children
//             c = 0..3 of those voxels are ONE run of 64 fine voxels: transposed through a wave-private LDS tile into 16-byte
//             stores of a long run.  B operand straight from the channels-last rows, the slice's weights in registers.
//   backward  dx[v][ci] = sum over 64 children and Cout: K = 64 * Cout, wave a of a workgroup takes the children of fine plane
//             a (a contiguous quarter of K), VG groups of 16 coarse voxels per pass so that a weight fragment fetched from L2 is
//             used VG times; the four partial tiles meet in LDS in a fixed order.
//   wgrad     dW[ci][co,abc] = sum_v x[v,ci] * dy[child(v,abc),co]: the one-pass scheme of linear_wgrad.hip.  For a fixed fine
//             row ab the children c of a coarse voxel are adjacent fine voxels, so the "token row" of a slice is the coarse row
//             (Cin) and CH adjacent child rows (CH * Cout); both operands go through LDS and are read with the transposing
//             ds_read (contraction index = voxel).  Workgroup partials [ci][c, co] in the workspace, then a fixed-order sum.
// Everything else (fp32 compute mode, other channel counts) runs on the plain vector kernels below, which index the same
// images element by element; their weight gradient writes partial blocks of the same layout for the same reduction.
// Expected bound: HBM on the fine tensor (written once forward, read once by each backward kernel).
#include "common.h"

#include <stdlib.h>

namespace {

constexpr int D4_THREADS = 256;

struct Dc4Params {
    const void* x; long long ldx;      // coarse [N, D, H, W, Cin]   (forward input / backward output dx)
    const void* wp;                    // packed image
    const float* bias;
    void* y; long long ldy;            // fine [N, 4D, 4H, 4W, Cout] (forward output / backward input dy)
    int N, D, H, W, Cin, Cout;
    int cb, nkb;                       // cout block width and k-blocks of the image
};

MSSEG_DEVFN u32x4_t ldg16(const void* p) { return *(const u32x4_t*)p; }

// element (m, k) of a msseg_pack_weights image (T = 1)
template <typename T> MSSEG_DEVFN float wimg(const T* wp, int cb, int nkb, int m, int k) {
    constexpr int EPC = DT<T>::EPC;
    const int blk = m / cb, row = m - blk * cb, kb = k / (4 * EPC), kr = k - kb * 4 * EPC, q = kr / EPC, e = kr - q * EPC;
    return DT<T>::ld(wp + ((((long long)blk * nkb + kb) * 4 + q) * cb + row) * EPC + e);
}

// fine voxel index of child abc of coarse voxel (n, d, h, w)
MSSEG_DEVFN long long child_voxel(const Dc4Params& p, long long n, int d, int h, int w, int abc) {
    return ((n * 4 * p.D + 4 * d + (abc >> 4)) * 4 * p.H + 4 * h + ((abc >> 2) & 3)) * 4 * p.W + 4 * w + (abc & 3);
}

// ---------------------------------------------------------------------------------------------------------
// plain vector kernels: any channel count, fp32 or bf16 storage, fp32 accumulation
// ---------------------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(D4_THREADS) void dc4_fwd_plain_kernel(const Dc4Params p) {
    const T* __restrict__ xg = (const T*)p.x;
    const T* __restrict__ wp = (const T*)p.wp;
    T* __restrict__ yg = (T*)p.y;
    const long long total = (long long)p.N * p.D * p.H * p.W * 64 * p.Cout;
    for (long long i = blockIdx.x * (long long)D4_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * D4_THREADS) {
        const int co = (int)(i % p.Cout);
        long long t = i / p.Cout;                       // fine voxel
        const long long fv = t;
        const int fw = (int)(t % (4 * p.W)); t /= 4 * p.W;
        const int fh = (int)(t % (4 * p.H)); t /= 4 * p.H;
        const int fd = (int)(t % (4 * p.D));
        const long long n = t / (4 * p.D);
        const int abc = ((fd & 3) * 4 + (fh & 3)) * 4 + (fw & 3);
        const long long cv = ((n * p.D + (fd >> 2)) * p.H + (fh >> 2)) * p.W + (fw >> 2);
        const T* xr = xg + cv * p.ldx;
        const int m = abc * p.Cout + co;
        float acc = p.bias ? p.bias[co] : 0.f;
        for (int ci = 0; ci < p.Cin; ++ci) acc = fmaf(DT<T>::ld(xr + ci), wimg<T>(wp, p.cb, p.nkb, m, ci), acc);
        DT<T>::st(yg + fv * p.ldy + co, acc);
    }
}

template <typename T> __global__ __launch_bounds__(D4_THREADS) void dc4_bwd_plain_kernel(const Dc4Params p) {
    const T* __restrict__ dyg = (const T*)p.y;
    const T* __restrict__ wp = (const T*)p.wp;
    T* __restrict__ dxg = (T*)p.x;
    const long long total = (long long)p.N * p.D * p.H * p.W * p.Cin;
    for (long long i = blockIdx.x * (long long)D4_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * D4_THREADS) {
        const int ci = (int)(i % p.Cin);
        long long t = i / p.Cin;
        const long long cv = t;
        const int w = (int)(t % p.W); t /= p.W;
        const int h = (int)(t % p.H); t /= p.H;
        const int d = (int)(t % p.D);
        const long long n = t / p.D;
        float acc = 0.f;
        for (int abc = 0; abc < 64; ++abc) {
            const T* dr = dyg + child_voxel(p, n, d, h, w, abc) * p.ldy;
            float s = 0.f;
            for (int co = 0; co < p.Cout; ++co) s = fmaf(DT<T>::ld(dr + co), wimg<T>(wp, p.cb, p.nkb, ci, abc * p.Cout + co), s);
            acc += s;
        }
        DT<T>::st(dxg + cv * p.ldx + ci, acc);
    }
}

// partial block of workgroup (slice ab = blockIdx.y, chunk = blockIdx.x): part[ab][chunk][ci][c * Cout + co], the voxels
// [chunk * per, (chunk + 1) * per) summed in order, 32 at a time
template <typename T> __global__ __launch_bounds__(D4_THREADS) void dc4_wgrad_plain_kernel(const Dc4Params p, float* part, long long per) {
    const T* __restrict__ xg = (const T*)p.x;
    const T* __restrict__ dyg = (const T*)p.y;
    const int ab = blockIdx.y, mw = 4 * p.Cout, PART = p.Cin * mw;
    const long long NV = (long long)p.N * p.D * p.H * p.W;
    const long long v0 = blockIdx.x * per, v1 = (v0 + per < NV) ? v0 + per : NV;
    float* out = part + ((long long)ab * gridDim.x + blockIdx.x) * PART;
    for (int i = threadIdx.x; i < PART; i += D4_THREADS) {
        const int ci = i / mw, m = i - ci * mw, c = m / p.Cout, co = m - c * p.Cout;
        float acc = 0.f;
        for (long long vb = v0; vb < v1; vb += 32) {
            const long long ve = vb + 32 < v1 ? vb + 32 : v1;
            float s = 0.f;
            for (long long v = vb; v < ve; ++v) {
                long long t = v;
                const int w = (int)(t % p.W); t /= p.W;
                const int h = (int)(t % p.H); t /= p.H;
                const int d = (int)(t % p.D);
                const long long n = t / p.D;
                s = fmaf(DT<T>::ld(xg + v * p.ldx + ci), DT<T>::ld(dyg + child_voxel(p, n, d, h, w, ab * 4 + c) * p.ldy + co), s);
            }
            acc += s;
        }
        out[i] = acc;
    }
}

// dw[ci][co][a][b][c] (+)= sum over the nwg partial blocks of slice (ab, child group) in a fixed order
struct Dc4RedParams {
    const float* part;
    float* dw;
    int Cin, Cout, CH, nwg, accumulate;
};
__global__ __launch_bounds__(D4_THREADS) void dc4_wgrad_reduce_kernel(const Dc4RedParams p) {
    const int mw = p.CH * p.Cout, PART = p.Cin * mw, ncg = 4 / p.CH;
    const int total = 16 * ncg * PART;
    for (int i = blockIdx.x * D4_THREADS + threadIdx.x; i < total; i += gridDim.x * D4_THREADS) {
        const int sl = i / PART, e = i - sl * PART;
        const float* src = p.part + (long long)sl * p.nwg * PART + e;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int w = 0;
        for (; w + 3 < p.nwg; w += 4) {
            s0 += src[(long long)w * PART]; s1 += src[(long long)(w + 1) * PART];
            s2 += src[(long long)(w + 2) * PART]; s3 += src[(long long)(w + 3) * PART];
        }
        for (; w < p.nwg; ++w) s0 += src[(long long)w * PART];
        const float tot = (s0 + s1) + (s2 + s3);
        const int ci = e / mw, m = e - ci * mw, cl = m / p.Cout, co = m - cl * p.Cout;
        const int ab = sl / ncg, c = (sl - ab * ncg) * p.CH + cl;
        float* o = p.dw + ((long long)ci * p.Cout + co) * 64 + ab * 4 + c;
        *o = p.accumulate ? *o + tot : tot;
    }
}

// ---------------------------------------------------------------------------------------------------------
// bf16 forward: weights of the slice in registers
// ---------------------------------------------------------------------------------------------------------
template <int KS, int NH>   // KS = ceil(Cin / 32) k-steps, NH cout tiles per slice
__global__ __launch_bounds__(D4_THREADS, 2) void dc4_fwd_kernel(const Dc4Params p) {
    constexpr int CS = NH * 16;                         // channels of a slice
    constexpr int RSB = CS * 2 + 16;                    // LDS bytes per fine voxel (16-byte pad: fewer write conflicts)
    constexpr int FV = 64;                              // fine voxels of a segment: 4 children of 16 coarse voxels
    constexpr int TILE_B = FV * RSB;
    constexpr int CPV = CS * 2 / 16;                    // 16-byte chunks per fine voxel
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * TILE_B];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    unsigned char* tile = lds + wave * TILE_B;
    const bf16_t* __restrict__ xg = (const bf16_t*)p.x;
    const int nsl = p.Cout / CS;
    const int ab = blockIdx.y / nsl, js = blockIdx.y - ab * nsl;
    const int cbase = js * CS;
    bf16_t* __restrict__ yg = (bf16_t*)p.y + cbase;

    u32x4_t af[4][NH][KS];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < NH; ++j)
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                const int m0 = (ab * 4 + c) * p.Cout + cbase + j * 16;
                const int blk = m0 / p.cb, row = m0 - blk * p.cb + r;
                af[c][j][k] = ldg16((const unsigned char*)p.wp + ((((long long)blk * KS + k) * 4 + q) * p.cb + row) * 16);
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
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                f32x4_t acc = bv[j];
#pragma unroll
                for (int k = 0; k < KS; ++k) mma_chunk<bf16_t>(acc, af[c][j][k], bx[k]);
                const bf16x4_t o = {(bf16_t)acc[0], (bf16_t)acc[1], (bf16_t)acc[2], (bf16_t)acc[3]};
                *(bf16x4_t*)(tile + (4 * r + c) * RSB + (j * 16 + q * 4) * 2) = o;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private tile: LDS ops of one wave execute in order
        const int ncv = (p.W - w0) < 16 ? (p.W - w0) : 16;   // valid coarse voxels of this segment
        const long long frow = ((n * 4 * p.D + 4 * d + (ab >> 2)) * 4 * p.H + 4 * h + (ab & 3)) * 4 * p.W + 4 * w0;
#pragma unroll
        for (int it = 0; it < (FV * CPV + 63) / 64; ++it) {
            const int ch = it * 64 + lane;
            const int fv = ch / CPV, part = ch - fv * CPV;
            if (ch < FV * CPV && fv < 4 * ncv) {
                const u32x4_t v = *(const u32x4_t*)(tile + fv * RSB + part * 16);
                *(u32x4_t*)(yg + (frow + fv) * p.ldy + part * 8) = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads are done before the next group's writes
    }
}

// ---------------------------------------------------------------------------------------------------------
// bf16 backward-data: wave a takes fine plane a (a quarter of K = 64 * Cout), VG groups of 16 coarse voxels per pass
// ---------------------------------------------------------------------------------------------------------
template <int NH, int COUT, int VG>   // NH = Cin / 16 row tiles
__global__ __launch_bounds__(D4_THREADS, 1) void dc4_bwd_kernel(const Dc4Params p) {
    constexpr int KSW = COUT / 2;                       // k-steps per wave: 16 children * COUT / 32
    __shared__ __attribute__((aligned(16))) float xch[3][NH][VG][64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const bf16_t* __restrict__ dyg = (const bf16_t*)p.y;
    const long long NV = (long long)p.N * p.D * p.H * p.W;
    const int k0 = wave * KSW;
    long long arow[NH];                                 // byte offset of this lane's piece of row tile j in k-block 0
#pragma unroll
    for (int j = 0; j < NH; ++j) {
        const int m0 = j * 16;
        const int blk = m0 / p.cb, row = m0 - blk * p.cb + r;
        arow[j] = (((long long)blk * p.nkb * 4 + q) * p.cb + row) * 16;
    }
    const long long kstep_b = (long long)4 * p.cb * 16;  // bytes between k-blocks of the image
    const long long groups = (NV + 16 * VG - 1) / (16 * VG);
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        long long fbase[VG];
        bool valid[VG];
#pragma unroll
        for (int s = 0; s < VG; ++s) {
            const long long v = (g * VG + s) * 16 + r;
            valid[s] = v < NV;
            long long t = valid[s] ? v : 0;
            const int w = (int)(t % p.W); t /= p.W;
            const int h = (int)(t % p.H); t /= p.H;
            const int d = (int)(t % p.D);
            const long long n = t / p.D;
            fbase[s] = child_voxel(p, n, d, h, w, 0) * p.ldy;
        }
        f32x4_t acc[NH][VG];
#pragma unroll
        for (int j = 0; j < NH; ++j)
#pragma unroll
            for (int s = 0; s < VG; ++s) acc[j][s] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int kk = 0; kk < KSW; ++kk) {
            const int ks = k0 + kk;
            const int c0 = ks * 32 + q * 8;             // a 16-byte chunk never straddles two children (COUT % 8 == 0)
            const int abc = c0 / COUT, co = c0 - abc * COUT;
            const long long off = (((long long)(abc >> 4) * 4 * p.H + ((abc >> 2) & 3)) * 4 * p.W + (abc & 3)) * p.ldy + co;
            u32x4_t af[NH], bx[VG];
#pragma unroll
            for (int j = 0; j < NH; ++j) af[j] = ldg16((const unsigned char*)p.wp + arow[j] + ks * kstep_b);
#pragma unroll
            for (int s = 0; s < VG; ++s) bx[s] = valid[s] ? ldg16(dyg + fbase[s] + off) : u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int s = 0; s < VG; ++s) mma_chunk<bf16_t>(acc[j][s], af[j], bx[s]);
        }
        if (wave > 0) {
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int s = 0; s < VG; ++s) *(f32x4_t*)xch[wave - 1][j][s][lane] = acc[j][s];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int s = 0; s < VG; ++s) {
                if (!valid[s]) continue;
                const long long v = (g * VG + s) * 16 + r;
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const f32x4_t a1 = *(const f32x4_t*)xch[0][j][s][lane], a2 = *(const f32x4_t*)xch[1][j][s][lane],
                                  a3 = *(const f32x4_t*)xch[2][j][s][lane];
                    const f32x4_t o = (acc[j][s] + a1) + (a2 + a3);
                    const bf16x4_t ob = {(bf16_t)o[0], (bf16_t)o[1], (bf16_t)o[2], (bf16_t)o[3]};
                    *(bf16x4_t*)((bf16_t*)p.x + v * p.ldx + j * 16 + q * 4) = ob;
                }
            }
        }
        __syncthreads();                                // wave 0 has read the exchange tiles before the next group's writes
    }
}

// ---------------------------------------------------------------------------------------------------------
// bf16 weight gradient: linear_wgrad.hip's one-pass kernel on gathered rows
// ---------------------------------------------------------------------------------------------------------
constexpr int TT = 128;            // coarse voxels per chunk
constexpr int RS = 96;             // LDS row pitch of a 32-channel block image (conflict-free transposing reads)
constexpr int BLK_BYTES = TT * RS;

struct Dc4WgParams {
    const void* x; long long ldx;      // coarse [NV][Cin]
    const void* dy; long long lddy;    // fine [N, 4D, 4H, 4W, Cout]
    float* part;                       // [slice][workgroup][ci][cl * Cout + co] fp32
    long long NV;
    int D, H, W, nchunks;
};

MSSEG_DEVFN bf16x4_t lds_tr_read(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) bf16x4_t*)(uintptr_t)(uint32_t)(uintptr_t)p);
}
MSSEG_DEVFN u32x4_t tr_frag(const unsigned char* base, int r0, int r1) {
    const bf16x4_t lo = lds_tr_read(base + r0), hi = lds_tr_read(base + r1);
    const bf16x8_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(u32x4_t, f);
}

template <int NTP, int NTQ, int CH>   // NTP = CH * Cout / 16 tiles of the gathered dy row, NTQ = Cin / 16, CH children per slice
__global__ __launch_bounds__(D4_THREADS, 1) void dc4_wgrad_kernel(const Dc4WgParams p) {
    constexpr int COUT = NTP * 16 / CH;
    constexpr int NBP = (NTP + 1) / 2, NBQ = (NTQ + 1) / 2;       // 32-channel block images
    constexpr int CHP = NTP * 2, CHQ = NTQ * 2;                   // 16-byte pieces per row
    constexpr int NLP = (TT * CHP + D4_THREADS - 1) / D4_THREADS; // staged pieces per thread
    constexpr int NLQ = (TT * CHQ + D4_THREADS - 1) / D4_THREADS;
    constexpr int PART = NTP * 16 * NTQ * 16;
    extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
    unsigned char* ldsP = smem;
    unsigned char* ldsQ = smem + NBP * BLK_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NCG = 4 / CH;
    const int ab = blockIdx.y / NCG, cg = blockIdx.y - ab * NCG;
    const unsigned char* qg = (const unsigned char*)p.x;

    u32x4_t sp[NLP], sq[NLQ];
    __shared__ unsigned fbase[2][TT];   // fine voxel (4d + a, 4h + b, 4w + cg * CH) of the chunk's coarse voxels (count < 2^31)
    auto fill_table = [&](int chunk, int sel) {
        if (tid < TT) {
            unsigned t = (unsigned)chunk * (unsigned)TT + (unsigned)tid;
            if ((long long)t >= p.NV) t = 0;
            const unsigned w = t % (unsigned)p.W; t /= (unsigned)p.W;
            const unsigned h = t % (unsigned)p.H; t /= (unsigned)p.H;
            const unsigned d = t % (unsigned)p.D, n = t / (unsigned)p.D;
            fbase[sel][tid] = ((n * 4u * p.D + 4u * d + (unsigned)(ab >> 2)) * 4u * p.H + 4u * h + (unsigned)(ab & 3)) * 4u * p.W +
                              4u * w + (unsigned)(cg * CH);
        }
    };
    auto fetch = [&](int chunk, int tsel) {
        const long long t0 = (long long)chunk * TT;
        const int rows = (p.NV - t0) < TT ? (int)(p.NV - t0) : TT;
        const unsigned char* qb = qg + t0 * p.ldx * 2;
#pragma unroll
        for (int it = 0; it < NLP; ++it) {
            const int i = tid + it * D4_THREADS, row = i / CHP, c = i - row * CHP;
            const unsigned ch = (unsigned)c * 8u;
            const unsigned cl = ch / (unsigned)COUT, co = ch - cl * (unsigned)COUT;
            const unsigned fv = fbase[tsel][row < TT ? row : 0] + cl;
            sp[it] = row < rows ? *(const u32x4_t*)((const unsigned char*)p.dy + ((unsigned long long)fv * (unsigned long long)p.lddy + co) * 2)
                                : u32x4_t{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int it = 0; it < NLQ; ++it) {
            const int i = tid + it * D4_THREADS, row = i / CHQ, c = i - row * CHQ;
            sq[it] = row < rows ? *(const u32x4_t*)(qb + ((long long)row * p.ldx * 2 + c * 16)) : u32x4_t{0u, 0u, 0u, 0u};
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int it = 0; it < NLP; ++it) {
            const int i = tid + it * D4_THREADS, row = i / CHP, c = i - row * CHP;
            if (row < TT) *(u32x4_t*)(ldsP + (c >> 2) * BLK_BYTES + row * RS + (c & 3) * 16) = sp[it];
        }
#pragma unroll
        for (int it = 0; it < NLQ; ++it) {
            const int i = tid + it * D4_THREADS, row = i / CHQ, c = i - row * CHQ;
            if (row < TT) *(u32x4_t*)(ldsQ + (c >> 2) * BLK_BYTES + row * RS + (c & 3) * 16) = sq[it];
        }
    };

    // transposing fragment reads: lane = 16 g + 4 qr + pc supplies row 8 g + 4 i + qr of the wave's 32 voxels, channels 4 pc ..
    // of a 16-channel tile (as linear_wgrad.hip)
    const int g = lane >> 4, qr = (lane >> 2) & 3, pc = lane & 3;
    int trow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) trow[i] = (wave * 32 + 8 * g + 4 * i + qr) * RS + pc * 8;

    f32x4_t acc[NTP][NTQ];
#pragma unroll
    for (int a = 0; a < NTP; ++a)
#pragma unroll
        for (int b = 0; b < NTQ; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    fill_table(blockIdx.x, 0);
    __syncthreads();
    if ((int)blockIdx.x < p.nchunks) fetch(blockIdx.x, 0);
    int tsel = 0;
    for (int chunk = blockIdx.x; chunk < p.nchunks; chunk += gridDim.x) {
        __syncthreads();                 // the previous chunk's fragment reads are done
        commit();
        tsel ^= 1;
        fill_table(chunk + gridDim.x, tsel);   // read by the fetch behind the next barrier
        __syncthreads();
        if (chunk + (int)gridDim.x < p.nchunks) fetch(chunk + gridDim.x, tsel);
        u32x4_t pf[NTP], qf[NTQ];
#pragma unroll
        for (int a = 0; a < NTP; ++a) pf[a] = tr_frag(ldsP + (a >> 1) * BLK_BYTES, trow[0] + (a & 1) * 32, trow[1] + (a & 1) * 32);
#pragma unroll
        for (int b = 0; b < NTQ; ++b) qf[b] = tr_frag(ldsQ + (b >> 1) * BLK_BYTES, trow[0] + (b & 1) * 32, trow[1] + (b & 1) * 32);
#pragma unroll
        for (int a = 0; a < NTP; ++a)
#pragma unroll
            for (int b = 0; b < NTQ; ++b) mma_chunk<bf16_t>(acc[a][b], pf[a], qf[b]);
    }

    // the four waves' partial sums (different voxels) meet in LDS as [wave][ci][m] and are added in a fixed order
    __syncthreads();                     // the images are dead
    float* xch = (float*)smem;
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int a = 0; a < NTP; ++a)
#pragma unroll
        for (int b = 0; b < NTQ; ++b)
            *(f32x4_t*)(xch + wave * PART + (b * 16 + r) * (NTP * 16) + a * 16 + q * 4) = acc[a][b];
    __syncthreads();
    float* out = p.part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * PART;
    for (int i = tid * 4; i < PART; i += D4_THREADS * 4) {
        const f32x4_t v0 = *(const f32x4_t*)(xch + i), v1 = *(const f32x4_t*)(xch + PART + i),
                      v2 = *(const f32x4_t*)(xch + 2 * PART + i), v3 = *(const f32x4_t*)(xch + 3 * PART + i);
        *(f32x4_t*)(out + i) = (v0 + v1) + (v2 + v3);
    }
}

template <int NTP, int NTQ, int CH> int launch_wgrad(const Dc4WgParams& p, int gx, hipStream_t stream) {
    constexpr int NBP = (NTP + 1) / 2, NBQ = (NTQ + 1) / 2;
    constexpr int PART = NTP * 16 * NTQ * 16;
    constexpr int lds = (NBP + NBQ) * BLK_BYTES > 4 * PART * 4 ? (NBP + NBQ) * BLK_BYTES : 4 * PART * 4;
    static_assert(lds <= 156 * 1024, "LDS budget");
    auto kern = dc4_wgrad_kernel<NTP, NTQ, CH>;
    static msseg_lds_attr_once attr;
    if (!attr.ensure((const void*)kern, lds)) MSSEG_FAIL(MSSEG_ELAUNCH, "deconv_k4s4_wgrad: cannot set dynamic LDS size %d", lds);
    MSSEG_KTIMED("dc4_wgrad_kernel", stream,
                 hipLaunchKernelGGL(kern, dim3(gx, 16 * (4 / CH)), dim3(D4_THREADS), lds, stream, p));
    MSSEG_CHECK_LAUNCH("deconv_k4s4_wgrad");
    return MSSEG_OK;
}

// ---- which path a call takes ----
bool aligned_bf16(int dtype, const void* coarse, long long ldc, const void* fine, long long ldf, int Cin, int Cout) {
    if (dtype != MSSEG_BF16) return false;
    return !((ldc % 8) || (ldf % 8) || ((uintptr_t)coarse & 15) || ((uintptr_t)fine & 15) || ldc < Cin || ldf < Cout);
}
// forward instantiation: k-steps, cout tiles per slice (4 * NH * KS weight fragments per lane <= 24)
bool fwd_cfg(int Cin, int Cout, int* ks, int* nh) {
    if (Cin % 8 || Cin > 96) return false;
    *ks = (Cin + 31) / 32;
    if (Cout % 48 == 0 && *ks <= 2) { *nh = 3; return true; }
    if (Cout % 32 == 0) { *nh = 2; return true; }
    return false;
}
bool square_fast(int Cin, int Cout) { return Cin == Cout && (Cin == 32 || Cin == 48 || Cin == 64 || Cin == 96); }

int grid_plain(long long total) {
    long long b = (total + D4_THREADS - 1) / D4_THREADS;
    const long long cap = (long long)msseg_num_cus() * 32;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

int check_shape(const char* what, int N, int D, int H, int W, int Cin, int Cout, int dtype) {
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "%s: bad dtype %d", what, dtype);
    if (N < 1 || D < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) MSSEG_FAIL(MSSEG_EINVAL, "%s: bad shape", what);
    const long long NV = (long long)N * D * H * W;
    if (NV > 0x7fffffffLL / 64) MSSEG_FAIL(MSSEG_EINVAL, "%s: more than 2^31 fine voxels", what);
    return MSSEG_OK;
}

}  // namespace

extern "C" {

int msseg_deconv_k4s4_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy, int N,
                          int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !wp || !y) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_fwd: null pointer");
    if (int rc = check_shape("deconv_k4s4_fwd", N, D, H, W, Cin, Cout, dtype)) return rc;
    if (ldx < Cin || ldy < Cout) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_fwd: leading dimension below the channel count");
    Dc4Params p{};
    p.x = x; p.ldx = ldx; p.wp = wp; p.bias = bias; p.y = y; p.ldy = ldy;
    p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.cb = msseg_cout_block(64 * Cout);
    p.nkb = (Cin + (dtype == MSSEG_F32 ? 15 : 31)) / (dtype == MSSEG_F32 ? 16 : 32);
    int ks = 0, nh = 0;
    if (aligned_bf16(dtype, x, ldx, y, ldy, Cin, Cout) && !((uintptr_t)wp & 15) && !(bias && ((uintptr_t)bias & 15)) &&
        fwd_cfg(Cin, Cout, &ks, &nh)) {
        const int slices = 16 * (Cout / (nh * 16));
        const long long groups = (long long)N * D * H * ((W + 15) / 16);
        long long gx = (groups + 3) / 4;
        // persistent above four rounds of two workgroups per CU.  A wave loads its 4 * NH * KS weight fragments once (24 KB at
        // 48 -> 48 against 6 KB of output per group): where that would leave a wave fewer than 8 groups, one resident round
        // (measured, tools/bench_deconv.py: 48 -> 48 @24^3 48.7 -> 44.1 us; 32 -> 32 @24^3 and 48 -> 48 @32^3 are faster on the
        // larger grid, 29.1 / 101.6 against 34.0 / 115.3 us)
        long long cap = (long long)msseg_num_cus() * 8 / slices;
        if (4 * nh * ks >= 24 && groups < cap * 4 * 8) cap = (long long)msseg_num_cus() * 2 / slices;
        if (cap < 1) cap = 1;
        if (gx > cap) gx = cap;
        dim3 grid((unsigned)gx, (unsigned)slices);
#define DC4_FWD(KS_, NH_)                                                                                          \
    if (ks == KS_ && nh == NH_) {                                                                                  \
        MSSEG_KTIMED("dc4_fwd_kernel", stream,                                                                      \
                     hipLaunchKernelGGL((dc4_fwd_kernel<KS_, NH_>), grid, dim3(D4_THREADS), 0, stream, p));        \
    } else
        DC4_FWD(1, 2) DC4_FWD(1, 3) DC4_FWD(2, 2) DC4_FWD(2, 3) DC4_FWD(3, 2) {}
#undef DC4_FWD
        MSSEG_CHECK_LAUNCH("deconv_k4s4_fwd");
        return MSSEG_OK;
    }
    const int gx = grid_plain((long long)N * D * H * W * 64 * Cout);
    if (dtype == MSSEG_F32) hipLaunchKernelGGL(dc4_fwd_plain_kernel<float>, dim3(gx), dim3(D4_THREADS), 0, stream, p);
    else hipLaunchKernelGGL(dc4_fwd_plain_kernel<bf16_t>, dim3(gx), dim3(D4_THREADS), 0, stream, p);
    MSSEG_CHECK_LAUNCH("deconv_k4s4_fwd");
    return MSSEG_OK;
}

int msseg_deconv_k4s4_bwd_data(const void* dy, long long lddy, const void* wp, void* dx, long long lddx, int N, int D, int H,
                               int W, int Cin, int Cout, int dtype, msseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dy || !wp || !dx) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_bwd_data: null pointer");
    if (int rc = check_shape("deconv_k4s4_bwd_data", N, D, H, W, Cin, Cout, dtype)) return rc;
    if (lddx < Cin || lddy < Cout) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_bwd_data: leading dimension below the channel count");
    Dc4Params p{};
    p.x = dx; p.ldx = lddx; p.wp = wp; p.y = (void*)dy; p.ldy = lddy;
    p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.cb = msseg_cout_block(Cin);
    p.nkb = (64 * Cout + (dtype == MSSEG_F32 ? 15 : 31)) / (dtype == MSSEG_F32 ? 16 : 32);
    if (aligned_bf16(dtype, dx, lddx, dy, lddy, Cin, Cout) && !((uintptr_t)wp & 15) && square_fast(Cin, Cout)) {
        const long long NV = (long long)N * D * H * W;
        const int vg = Cin == 96 ? 2 : 4;
        long long gx = (NV + 16 * vg - 1) / (16 * vg);
        const long long cap = (long long)msseg_num_cus() * 8;
        if (gx > cap) gx = cap;
        dim3 grid((unsigned)gx);
#define DC4_BWD(NH_, COUT_, VG_)                                                                                   \
    if (Cin == COUT_) {                                                                                            \
        MSSEG_KTIMED("dc4_bwd_kernel", stream,                                                                      \
                     hipLaunchKernelGGL((dc4_bwd_kernel<NH_, COUT_, VG_>), grid, dim3(D4_THREADS), 0, stream, p)); \
    } else
        DC4_BWD(2, 32, 4) DC4_BWD(3, 48, 4) DC4_BWD(4, 64, 4) DC4_BWD(6, 96, 2) {}
#undef DC4_BWD
        MSSEG_CHECK_LAUNCH("deconv_k4s4_bwd_data");
        return MSSEG_OK;
    }
    const int gx = grid_plain((long long)N * D * H * W * Cin);
    if (dtype == MSSEG_F32) hipLaunchKernelGGL(dc4_bwd_plain_kernel<float>, dim3(gx), dim3(D4_THREADS), 0, stream, p);
    else hipLaunchKernelGGL(dc4_bwd_plain_kernel<bf16_t>, dim3(gx), dim3(D4_THREADS), 0, stream, p);
    MSSEG_CHECK_LAUNCH("deconv_k4s4_bwd_data");
    return MSSEG_OK;
}

int msseg_deconv_k4s4_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw, int N, int D, int H, int W,
                            int Cin, int Cout, int accumulate, void* workspace, size_t workspace_bytes, int dtype,
                            msseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !dy || !dw || !workspace) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_wgrad: null pointer");
    if (int rc = check_shape("deconv_k4s4_wgrad", N, D, H, W, Cin, Cout, dtype)) return rc;
    if (ldx < Cin || lddy < Cout) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_wgrad: leading dimension below the channel count");
    if ((uintptr_t)workspace & 15) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_wgrad: workspace alignment");
    const long long NV = (long long)N * D * H * W;
    const size_t img_bytes = (size_t)Cin * 64 * Cout * 4;         // all slices of one workgroup column
    const size_t fit = workspace_bytes / img_bytes;
    if (fit < 1) MSSEG_FAIL(MSSEG_EWORKSPACE, "deconv_k4s4_wgrad: workspace %zu B too small (need >= %zu)", workspace_bytes, img_bytes);
    Dc4RedParams r{};
    r.part = (const float*)workspace; r.dw = dw; r.Cin = Cin; r.Cout = Cout; r.accumulate = accumulate;
    if (aligned_bf16(dtype, x, ldx, dy, lddy, Cin, Cout) && square_fast(Cin, Cout)) {
        Dc4WgParams p{};
        p.x = x; p.ldx = ldx; p.dy = dy; p.lddy = lddy; p.part = (float*)workspace; p.NV = NV;
        p.D = D; p.H = H; p.W = W; p.nchunks = (int)((NV + TT - 1) / TT);
        const int ch = Cin == 96 ? 1 : Cin == 64 ? 2 : 4;
        const int slices = 16 * (4 / ch);
        int gx = msseg_num_cus() / slices;
        if (gx > (p.nchunks + 1) / 2) gx = (p.nchunks + 1) / 2;
        if ((size_t)gx > fit) gx = (int)fit;
        if (gx < 1) gx = 1;
        int rc = MSSEG_EINVAL;
        switch (Cin) {
            case 32: rc = launch_wgrad<8, 2, 4>(p, gx, stream); break;
            case 48: rc = launch_wgrad<12, 3, 4>(p, gx, stream); break;
            case 64: rc = launch_wgrad<8, 4, 2>(p, gx, stream); break;
            case 96: rc = launch_wgrad<6, 6, 1>(p, gx, stream); break;
        }
        if (rc) return rc;
        r.CH = ch; r.nwg = gx;
    } else {
        Dc4Params p{};
        p.x = x; p.ldx = ldx; p.y = (void*)dy; p.ldy = lddy;
        p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
        long long gx = (NV + 63) / 64;                            // at least 64 voxels per partial block
        const long long cap = msseg_num_cus() / 16 > 0 ? msseg_num_cus() / 16 * 4 : 4;
        if (gx > cap) gx = cap;
        if ((size_t)gx > fit) gx = (long long)fit;
        if (gx < 1) gx = 1;
        const long long per = (NV + gx - 1) / gx;
        dim3 grid((unsigned)gx, 16);
        if (dtype == MSSEG_F32) hipLaunchKernelGGL(dc4_wgrad_plain_kernel<float>, grid, dim3(D4_THREADS), 0, stream, p, (float*)workspace, per);
        else hipLaunchKernelGGL(dc4_wgrad_plain_kernel<bf16_t>, grid, dim3(D4_THREADS), 0, stream, p, (float*)workspace, per);
        MSSEG_CHECK_LAUNCH("deconv_k4s4_wgrad");
        r.CH = 4; r.nwg = (int)gx;
    }
    int rb = (Cin * 64 * Cout + D4_THREADS - 1) / D4_THREADS;
    if (rb > 4096) rb = 4096;
    hipLaunchKernelGGL(dc4_wgrad_reduce_kernel, dim3(rb), dim3(D4_THREADS), 0, stream, r);
    MSSEG_CHECK_LAUNCH("deconv_k4s4_wgrad_reduce");
    return MSSEG_OK;
}

}  // extern "C"
