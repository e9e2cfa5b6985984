// ConvTranspose3d k = s = 4 for gfx950: the last up block of Swin-UNETR with patch size 4 (hidden -> hidden, vol/4 -> vol).
//
//   y[n, 4d+a, 4h+b, 4w+c, co] = bias[co] + sum_ci x[n,d,h,w,ci] * W[ci,co,a,b,c]          64 children per coarse voxel
//
// Weight images are the ones of msseg_pack_weights (T = 1), as for k2 s2 with 8 -> 64:
//   forward / weight gradient   M = abc * Cout + co (abc = (a*4 + b)*4 + c), K = ci
//   input gradient              M = ci, K = abc * Cout + co
//
// bf16 fast path (Cin = Cout in {32, 48, 64, 96}; the forward takes a few more shapes), same scheme as deconv_k2s2_gen.hip:
//   forward   deconv_sliced_fwd_kernel<S = 4> (deconv_sliced.h, shared with k2 s2): grid.y slices the output by (fine row ab,
//             cout slice); the four children c = 0..3 of a wave's 16 coarse voxels are ONE run of 64 fine voxels.
//   backward  dx[v][ci] = sum over 64 children and Cout: K = 64 * Cout, wave a of a workgroup takes the children of fine plane
//             a (a contiguous quarter of K), VG groups of 16 coarse voxels per pass so that a weight fragment fetched from L2 is
//             used VG times; the four partial tiles meet in LDS in a fixed order.
//   wgrad     dW[ci][co,abc] = sum_v x[v,ci] * dy[child(v,abc),co]: the one-pass kernel of wgrad_onepass.h with the row source
//             RowsDeconvK4.  For a fixed fine row ab the children c of a coarse voxel are adjacent fine voxels, so the "token
//             row" of a slice is the coarse row (Cin) and CH adjacent child rows (CH * Cout).  Workgroup partials [ci][c, co]
//             in the workspace, then a fixed-order sum.
// Everything else (fp32 compute mode, other channel counts) runs on the plain vector kernels below, which index the same
// images element by element; their weight gradient writes partial blocks of the same layout for the same reduction.
// Expected bound: HBM on the fine tensor (written once forward, read once by each backward kernel).
#include "deconv_sliced.h"
#include "wgrad_onepass.h"

#include <stdlib.h>

namespace {

constexpr int D4_THREADS = 256;

// element (m, k) of a msseg_pack_weights image (T = 1)
template <typename T> MSSEG_DEVFN float wimg(const T* wp, int cb, int nkb, int m, int k) {
    constexpr int EPC = DT<T>::EPC;
    const int blk = m / cb, row = m - blk * cb, kb = k / (4 * EPC), kr = k - kb * 4 * EPC, q = kr / EPC, e = kr - q * EPC;
    return DT<T>::ld(wp + ((((long long)blk * nkb + kb) * 4 + q) * cb + row) * EPC + e);
}

// fine voxel index of child abc of coarse voxel (n, d, h, w)
MSSEG_DEVFN long long child_voxel(const DeconvParams& p, long long n, int d, int h, int w, int abc) {
    return ((n * 4 * p.D + 4 * d + (abc >> 4)) * 4 * p.H + 4 * h + ((abc >> 2) & 3)) * 4 * p.W + 4 * w + (abc & 3);
}

// ---------------------------------------------------------------------------------------------------------
// plain vector kernels: any channel count, fp32 or bf16 storage, fp32 accumulation
// ---------------------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(D4_THREADS) void dc4_fwd_plain_kernel(const DeconvParams p) {
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

template <typename T> __global__ __launch_bounds__(D4_THREADS) void dc4_bwd_plain_kernel(const DeconvParams p) {
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
template <typename T> __global__ __launch_bounds__(D4_THREADS) void dc4_wgrad_plain_kernel(const DeconvParams p, float* part, long long per) {
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
// bf16 backward-data: wave a takes fine plane a (a quarter of K = 64 * Cout), VG groups of 16 coarse voxels per pass
// ---------------------------------------------------------------------------------------------------------
template <int NH, int COUT, int VG>   // NH = Cin / 16 row tiles
__global__ __launch_bounds__(D4_THREADS, 1) void dc4_bwd_kernel(const DeconvParams p) {
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
        arow[j] = wimg_frag_off(blk, p.nkb, 0, q, p.cb, row);
    }
    const long long kstep_b = wimg_kblock_bytes(p.cb);
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

// ---- which path a call takes ----
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
    DeconvParams p{};
    p.x = x; p.ldx = ldx; p.wp = wp; p.bias = bias; p.y = y; p.ldy = ldy;
    p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.cb = msseg_cout_block(64 * Cout);
    p.nkb = (Cin + (dtype == MSSEG_F32 ? 15 : 31)) / (dtype == MSSEG_F32 ? 16 : 32);
    int ks = 0, nh = 0;
    if (msseg_aligned_bf16(dtype, x, ldx, Cin, y, ldy, Cout) && !((uintptr_t)wp & 15) && !(bias && ((uintptr_t)bias & 15)) &&
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
#define DC4_FWD(KS_, NH_)                                                                                                    \
    if (ks == KS_ && nh == NH_) {                                                                                            \
        MSSEG_KTIMED("dc4_fwd_kernel", stream,                                                                                \
                     hipLaunchKernelGGL((deconv_sliced_fwd_kernel<4, KS_, NH_, 4>), grid, dim3(DECONV_THREADS), 0, stream, p)); \
    } else
        DC4_FWD(1, 2) DC4_FWD(1, 3) DC4_FWD(2, 2) DC4_FWD(2, 3) DC4_FWD(3, 2) {}
#undef DC4_FWD
        MSSEG_CHECK_LAUNCH("deconv_k4s4_fwd");
        return MSSEG_OK;
    }
    const int gx = grid_plain((long long)N * D * H * W * 64 * Cout);
    for_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(dc4_fwd_plain_kernel<typename decltype(t)::type>, dim3(gx), dim3(D4_THREADS), 0, stream, p);
    });
    MSSEG_CHECK_LAUNCH("deconv_k4s4_fwd");
    return MSSEG_OK;
}

int msseg_deconv_k4s4_bwd_data(const void* dy, long long lddy, const void* wp, void* dx, long long lddx, int N, int D, int H,
                               int W, int Cin, int Cout, int dtype, msseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!dy || !wp || !dx) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_bwd_data: null pointer");
    if (int rc = check_shape("deconv_k4s4_bwd_data", N, D, H, W, Cin, Cout, dtype)) return rc;
    if (lddx < Cin || lddy < Cout) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k4s4_bwd_data: leading dimension below the channel count");
    DeconvParams p{};
    p.x = dx; p.ldx = lddx; p.wp = wp; p.y = (void*)dy; p.ldy = lddy;
    p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.cb = msseg_cout_block(Cin);
    p.nkb = (64 * Cout + (dtype == MSSEG_F32 ? 15 : 31)) / (dtype == MSSEG_F32 ? 16 : 32);
    if (msseg_aligned_bf16(dtype, dx, lddx, Cin, dy, lddy, Cout) && !((uintptr_t)wp & 15) && square_fast(Cin, Cout)) {
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
    for_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(dc4_bwd_plain_kernel<typename decltype(t)::type>, dim3(gx), dim3(D4_THREADS), 0, stream, p);
    });
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
    if (msseg_aligned_bf16(dtype, x, ldx, Cin, dy, lddy, Cout) && square_fast(Cin, Cout)) {
        // the one-pass kernel of wgrad_onepass.h: the "token row" of a slice is the coarse row (Cin) and CH adjacent child rows
        LwgParams p{};
        p.x = x; p.ldx = ldx; p.dy = dy; p.lddy = lddy; p.part = (float*)workspace; p.NV = NV;
        p.D = D; p.H = H; p.W = W; p.nchunks = (int)((NV + LWG_TT - 1) / LWG_TT);
        const int ch = Cin == 96 ? 1 : Cin == 64 ? 2 : 4;
        const int slices = 16 * (4 / ch);
        const int gx = lwg_grid_x(slices, p.nchunks, fit);
        const char* who = "deconv_k4s4_wgrad";
        int rc = MSSEG_EINVAL;
        switch (Cin) {   // <NTP = CH * Cout / 16, NTQ = Cin / 16>
            case 32: rc = lwg_launch<8, 2, RowsDeconvK4<4, 32>>(p, gx, slices, who, stream); break;
            case 48: rc = lwg_launch<12, 3, RowsDeconvK4<4, 48>>(p, gx, slices, who, stream); break;
            case 64: rc = lwg_launch<8, 4, RowsDeconvK4<2, 64>>(p, gx, slices, who, stream); break;
            case 96: rc = lwg_launch<6, 6, RowsDeconvK4<1, 96>>(p, gx, slices, who, stream); break;
        }
        if (rc) return rc;
        r.CH = ch; r.nwg = gx;
    } else {
        DeconvParams p{};
        p.x = x; p.ldx = ldx; p.y = (void*)dy; p.ldy = lddy;
        p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
        long long gx = (NV + 63) / 64;                            // at least 64 voxels per partial block
        const long long cap = msseg_num_cus() / 16 > 0 ? msseg_num_cus() / 16 * 4 : 4;
        if (gx > cap) gx = cap;
        if ((size_t)gx > fit) gx = (long long)fit;
        if (gx < 1) gx = 1;
        const long long per = (NV + gx - 1) / gx;
        dim3 grid((unsigned)gx, 16);
        for_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL(dc4_wgrad_plain_kernel<typename decltype(t)::type>, grid, dim3(D4_THREADS), 0, stream, p,
                               (float*)workspace, per);
        });
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
