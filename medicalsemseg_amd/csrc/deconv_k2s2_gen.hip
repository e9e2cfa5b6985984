// ConvTranspose3d k = s = 2 (bf16) for the channel counts the register-resident kernels of deconv_k2s2.hip do not hold:
// the transposed convolutions of Swin-UNETR's UnetrUpBlocks (/root/reference/models/segmentors/swin_unetr.py:93-128:
// 768 -> 384 @3^3, 384 -> 192 @6^3, 192 -> 96 @12^3, 96 -> 48 @24^3, 48 -> 48 @48^3) and the deep UpCat levels of MONAI
// BasicUNet (256 -> 128 @6^3, 128 -> 64 @12^3).  The generic implicit-GEMM path ran them as flat GEMMs through LDS-staged
// 256-voxel tiles, one 32-channel stage after the other (forward 52 us, input gradient 55-97 us per launch for 0.1-2 GFLOP;
// five + five launches = 0.64 ms of the Swin-UNETR step).
//
// Same scheme as deconv_k2s2.hip / linear_regw.hip -- a wave takes 16 coarse voxels, its B operand comes straight from
// global memory (a channels-last row IS the operand layout), the weights it needs live in registers -- with the output
// sliced over grid.y so that any channel count fits the register file:
//   forward   deconv_sliced_fwd_kernel<S = 2> (deconv_sliced.h, shared with k4 s4): slice = (fine row pair ab, cout slice): the
//             two children (ab, c = 0 / 1) of 16 coarse voxels form ONE fine row segment of 32 voxels, transposed through a
//             wave-private LDS tile into coalesced 16-byte stores.
//   backward  dx[v][ci] = sum over the 8 children and Cout: K = 8 * Cout is split over the FOUR WAVES of a workgroup (every
//             wave gathers its k-steps from the child rows -- a 16-byte chunk never straddles two children), the partial
//             tiles meet in LDS in a fixed order (deterministic); slice = Cin tiles.  Output: bf16 dx, or the fp32 block
//             layout of the small-grid finish kernels (conv3d_k3_small.hip: [Cin / 4][voxel][4]), whose k3s_bwd_unit_kernel
//             then runs the receiving conv + InstanceNorm + LeakyReLU unit's whole backward in one launch.
// Bound: HBM on the 96^3 / 48^3 outputs (8x the input voxels written / read once), launch latency below.
#include "deconv_sliced.h"
#include "k3pp.h"

namespace {

constexpr int DG_THREADS = 256;

// ---------------------------------------------------------------------------------------------------------
// backward-data: the four waves split K = 8 * Cout
// ---------------------------------------------------------------------------------------------------------
template <int KSW, int NH, bool PART>   // KSW = Cout / 16 k-steps per wave, NH Cin tiles per slice
__global__ __launch_bounds__(DG_THREADS, 2) void dcg_bwd_kernel(const DeconvParams p) {
    __shared__ __attribute__((aligned(16))) float xch[3][NH][64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int mbase = blockIdx.y * NH * 16;
    const int kstot = 4 * KSW;                          // k-steps of the packed image (K = 8 * Cout = 128 * KSW)
    const int k0 = wave * KSW;
    const bf16_t* __restrict__ dyg = (const bf16_t*)p.y;
    const long long NV = (long long)p.N * p.D * p.H * p.W;

    u32x4_t af[NH][KSW];
#pragma unroll
    for (int j = 0; j < NH; ++j)
#pragma unroll
        for (int k = 0; k < KSW; ++k) {
            const int m0 = mbase + j * 16;
            const int blk = m0 / p.cb, row = m0 - blk * p.cb + r;
            af[j][k] = ldg16((const unsigned char*)p.wp + wimg_frag_off(blk, kstot, k0 + k, q, p.cb, row));
        }
    int off[KSW];                                       // this lane's chunk of k-step k0 + k, relative to fine voxel (2d, 2h, 2w)
#pragma unroll
    for (int k = 0; k < KSW; ++k) {
        const int c0 = (k0 + k) * 32 + q * 8;
        const int abc = c0 / p.Cout, co = c0 - abc * p.Cout;
        off[k] = (int)((((long long)(abc >> 2) * 2 * p.H + ((abc >> 1) & 1)) * 2 * p.W + (abc & 1)) * p.ldy) + co;
    }
    const long long groups = (NV + 15) >> 4;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long v = g * 16 + r;
        const bool valid = v < NV;
        long long t = valid ? v : 0;
        const int w = (int)(t % p.W); t /= p.W;
        const int h = (int)(t % p.H); t /= p.H;
        const int d = (int)(t % p.D);
        const long long n = t / p.D;
        const long long fbase = ((((n * 2 * p.D + 2 * d) * 2 * p.H + 2 * h) * 2 * p.W) + 2 * w) * p.ldy;
        u32x4_t bx[KSW];
#pragma unroll
        for (int k = 0; k < KSW; ++k) bx[k] = valid ? ldg16(dyg + fbase + off[k]) : u32x4_t{0u, 0u, 0u, 0u};
        f32x4_t acc[NH];
#pragma unroll
        for (int j = 0; j < NH; ++j) {
            acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KSW; ++k) mma_chunk<bf16_t>(acc[j], af[j][k], bx[k]);
        }
        if (wave > 0) {
#pragma unroll
            for (int j = 0; j < NH; ++j) *(f32x4_t*)xch[wave - 1][j][lane] = acc[j];
        }
        __syncthreads();
        if (wave == 0 && valid) {
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                const f32x4_t a1 = *(const f32x4_t*)xch[0][j][lane], a2 = *(const f32x4_t*)xch[1][j][lane], a3 = *(const f32x4_t*)xch[2][j][lane];
                const f32x4_t o = (acc[j] + a1) + (a2 + a3);
                const int m = mbase + j * 16 + q * 4;
                if constexpr (PART) {
                    *(f32x4_t*)(p.part + ((long long)(m >> 2) * NV + v) * 4) = o;
                } else {
                    const bf16x4_t ob = {(bf16_t)o[0], (bf16_t)o[1], (bf16_t)o[2], (bf16_t)o[3]};
                    *(bf16x4_t*)((bf16_t*)p.x + v * p.ldx + m) = ob;
                }
            }
        }
        __syncthreads();                                // wave 0 has read the exchange tiles before the next group's writes
    }
}

// forward instantiation for a shape: k-steps, cout tiles per slice, children per slice (weight fragments per lane <= 24)
struct FwdCfg { int ks, nh, ch; };
bool fwd_cfg(int Cin, int Cout, FwdCfg* c) {
    const int ks = (Cin + 31) / 32;
    static const FwdCfg table[] = {{2, 3, 2}, {3, 3, 2}, {4, 2, 2}, {6, 2, 2}, {8, 1, 2}, {12, 1, 2}, {24, 1, 1}};
    for (const FwdCfg& t : table)
        if (t.ks == ks && Cout % (t.nh * 16) == 0) { *c = t; return true; }
    return false;
}

// backward instantiation: k-steps per wave (Cout / 16), Cin tiles per slice
struct BwdCfg { int ksw, nh; };
bool bwd_cfg(int Cin, int Cout, BwdCfg* c) {
    if (Cout % 16 || Cin % 16) return false;
    static const BwdCfg table[] = {{3, 3}, {6, 4}, {12, 2}, {24, 1}, {8, 2}, {4, 4}};
    for (const BwdCfg& t : table)
        if (t.ksw == Cout / 16 && (Cin / 16) % t.nh == 0) { *c = t; return true; }
    return false;
}

}  // namespace

bool msseg_deconv2g_fwd_eligible(int dtype, int Cin, int Cout, const void* coarse, long long ldc, const void* fine,
                                 long long ldf, const float* bias) {
    FwdCfg c;
    if (!msseg_aligned_bf16(dtype, coarse, ldc, Cin, fine, ldf, Cout) || Cin % 8 || Cout % 16) return false;
    if (bias && ((uintptr_t)bias & 15)) return false;
    return fwd_cfg(Cin, Cout, &c);
}

int msseg_deconv2g_fwd_launch(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy, int N,
                              int D, int H, int W, int Cin, int Cout, hipStream_t stream) {
    FwdCfg c;
    if (!fwd_cfg(Cin, Cout, &c)) MSSEG_FAIL(MSSEG_EINVAL, "deconv2g_fwd: shape %d -> %d has no instantiation", Cin, Cout);
    DeconvParams p{};
    p.x = x; p.ldx = ldx; p.wp = wp; p.bias = bias; p.y = y; p.ldy = ldy;
    p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.cb = msseg_cout_block(8 * Cout);
    const int slices = (8 / c.ch) * (Cout / (c.nh * 16));
    const long long groups = (long long)N * D * H * ((W + 15) / 16);
    long long gx = (groups + 3) / 4;
    long long cap = (long long)msseg_num_cus() * 4 / slices;
    if (cap < 1) cap = 1;
    if (gx > cap) gx = cap;
    dim3 grid((unsigned)gx, (unsigned)slices);
#define DCG_FWD(KS_, NH_, CH_)                                                                                         \
    if (c.ks == KS_ && c.nh == NH_ && c.ch == CH_) {                                                                   \
        MSSEG_KTIMED("dcg_fwd_kernel", stream,                                                                          \
                     hipLaunchKernelGGL((deconv_sliced_fwd_kernel<2, KS_, NH_, CH_>), grid, dim3(DG_THREADS), 0, stream, p)); \
    } else
    DCG_FWD(2, 3, 2) DCG_FWD(3, 3, 2) DCG_FWD(4, 2, 2) DCG_FWD(6, 2, 2) DCG_FWD(8, 1, 2) DCG_FWD(12, 1, 2) DCG_FWD(24, 1, 1) {}
#undef DCG_FWD
    MSSEG_CHECK_LAUNCH("deconv2g_fwd");
    return MSSEG_OK;
}

bool msseg_deconv2g_bwd_eligible(int dtype, int Cin, int Cout, const void* coarse, long long ldc, const void* fine,
                                 long long ldf) {
    BwdCfg c;
    if (coarse == nullptr) {   // partial-sum form: no coarse tensor
        if (dtype != MSSEG_BF16 || (ldf % 8) || ((uintptr_t)fine & 15) || ldf < Cout) return false;
    } else if (!msseg_aligned_bf16(dtype, coarse, ldc, Cin, fine, ldf, Cout) || (ldc % 4)) {
        return false;
    }
    return bwd_cfg(Cin, Cout, &c);
}

// dx (bf16, part == nullptr) or part[Cin / 4][N*D*H*W][4] (fp32) = the input gradient of ConvTranspose3d k2 s2
int msseg_deconv2g_bwd_launch(const void* dy, long long lddy, const void* wp, void* dx, long long lddx, float* part, int N,
                              int D, int H, int W, int Cin, int Cout, hipStream_t stream) {
    BwdCfg c;
    if (!bwd_cfg(Cin, Cout, &c)) MSSEG_FAIL(MSSEG_EINVAL, "deconv2g_bwd: shape %d -> %d has no instantiation", Cin, Cout);
    if ((long long)(2 * H) * (2 * W) * 2 * lddy > 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "deconv2g_bwd: fine plane too large");
    DeconvParams p{};
    p.x = dx; p.ldx = lddx; p.wp = wp; p.y = (void*)dy; p.ldy = lddy; p.part = part;
    p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
    p.cb = msseg_cout_block(Cin);
    const int slices = Cin / (c.nh * 16);
    const long long groups = ((long long)N * D * H * W + 15) / 16;
    long long gx = groups;
    long long cap = (long long)msseg_num_cus() * 8 / slices;   // persistent above two rounds of two workgroups per CU
    if (cap < 1) cap = 1;
    if (gx > cap) gx = cap;
    dim3 grid((unsigned)gx, (unsigned)slices);
#define DCG_BWD(KSW_, NH_)                                                                                                     \
    if (c.ksw == KSW_ && c.nh == NH_) {                                                                                        \
        if (part) {                                                                                                            \
            MSSEG_KTIMED("dcg_bwd_kernel", stream,                                                                              \
                         hipLaunchKernelGGL((dcg_bwd_kernel<KSW_, NH_, true>), grid, dim3(DG_THREADS), 0, stream, p));         \
        } else {                                                                                                               \
            MSSEG_KTIMED("dcg_bwd_kernel", stream,                                                                              \
                         hipLaunchKernelGGL((dcg_bwd_kernel<KSW_, NH_, false>), grid, dim3(DG_THREADS), 0, stream, p));        \
        }                                                                                                                      \
    } else
    DCG_BWD(3, 3) DCG_BWD(6, 4) DCG_BWD(12, 2) DCG_BWD(24, 1) DCG_BWD(8, 2) DCG_BWD(4, 4) {}
#undef DCG_BWD
    MSSEG_CHECK_LAUNCH("deconv2g_bwd");
    return MSSEG_OK;
}

extern "C" {

/* 1 when msseg_deconv_k2s2_bwd_partials takes the shape (bf16, channel counts with an instantiation) */
int msseg_deconv_k2s2_bwd_partials_ok(int Cin, int Cout, int dtype) {
    BwdCfg c;
    return (dtype == MSSEG_BF16 && bwd_cfg(Cin, Cout, &c) && Cin % 32 == 0) ? 1 : 0;
}

/* input gradient of ConvTranspose3d k2 s2 as ONE fp32 stage group in the layout of msseg_conv3d_k3_small_partials
 * (part[Cin / 4][N*D*H*W][4]): msseg_conv3d_k3_small_bwd_finish(part, 1, ...) then stores it, or runs the whole backward
 * of the conv + InstanceNorm + LeakyReLU unit whose activation the transposed conv read.  dy: fine [N, 2D, 2H, 2W, Cout];
 * wp: the backward image of msseg_pack_weights (M = Cin, K = 8 * Cout). */
int msseg_deconv_k2s2_bwd_partials(const void* dy, long long lddy, const void* wp, float* part, size_t part_bytes, int N,
                                   int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream) {
    if (!dy || !wp || !part) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_partials: null pointer");
    if (!msseg_deconv_k2s2_bwd_partials_ok(Cin, Cout, dtype) || !msseg_deconv2g_bwd_eligible(dtype, Cin, Cout, nullptr, 0, dy, lddy))
        MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_partials: shape %d -> %d / alignment not supported", Cin, Cout);
    const long long NV = (long long)N * D * H * W;
    if (N < 1 || D < 1 || H < 1 || W < 1 || NV > 0x7fffffffLL / 8) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_partials: bad voxel count");
    if (((uintptr_t)wp & 15) || ((uintptr_t)part & 15)) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_partials: 16-byte alignment");
    if (part_bytes < (size_t)NV * Cin * sizeof(float))
        MSSEG_FAIL(MSSEG_EWORKSPACE, "deconv_k2s2_bwd_partials: workspace %zu B < %zu B", part_bytes, (size_t)NV * Cin * sizeof(float));
    return msseg_deconv2g_bwd_launch(dy, lddy, wp, nullptr, 0, part, N, D, H, W, Cin, Cout, (hipStream_t)stream);
}

}  // extern "C"
