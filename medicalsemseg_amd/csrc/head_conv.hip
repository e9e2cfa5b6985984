// The segmentation head: a 1x1x1 convolution with <= 4 output channels as streaming passes (HBM-bound) -- forward, forward
// on the raw conv output of the last conv+norm unit, and the backward fused with that unit's InstanceNorm-backward sums.
#include "channel_reduce.h"

namespace {

// Input gradient of the segmentation head (1x1x1 conv, <= 4 classes) fused with the InstanceNorm-backward sums of the
// layer whose activation a = lrelu(IN(x)) feeds the head: da[v][c] = T(sum_k dy[v][k] * w[k][c]) and
// (sum dz, sum dz * xhat), dz = da * lrelu'(pre-activation recomputed from x).  A streaming pass (thread = voxel x
// 16-byte channel chunk) with the reduction scheme of instnorm_kernel<MODE 1>; replaces a 16-wide MFMA column block fed
// with three real rows, and reads neither the packed weights nor the stored activation.
struct HeadBwdParams {
    const void* dy; long long lddy;
    const float* w;                      // [Cout][C] fp32
    const void* x; long long ldx;        // raw conv output of the receiving layer
    const float* stats; const float* gamma; const float* beta;
    void* da; long long ldda;
    long long S; int C, Cout; float eps, slope;
    int groups, rows_par; long long rows_per_block;
    float* ws;
    int want_dw;                         // also accumulate dW[k][c] = sum_v dy[v][k] * a[v][c], a = T(lrelu(IN(x))) recomputed
};

// second step of the head backward: rows ws[(n * nblk + b)][C][nper] (nper = 2, or 6 with the weight gradient) ->
// red[n][c][0..1], dbeta / dgamma (+)= sum_n, dW[k][c] (+)= sum_{n, b} -- one block, fixed order (bit-reproducible)
struct HeadFinArgs {
    const float* ws; int N, nblk, C, nper, Cout; float* red; float* dbeta; float* dgamma; float* dw; int acc_norm, acc_dw;
};
__global__ __launch_bounds__(256) void head_finalize_kernel(const HeadFinArgs a) {
    __shared__ __attribute__((aligned(16))) float fin[256 * 4 + 64 * 6];
    __shared__ float tot_n[64 * 6];
    const int L = a.C * a.nper;      // <= 64 * 6 floats, a multiple of 4
    for (int o = threadIdx.x; o < L; o += 256) tot_n[o] = 0.f;
    for (int n = 0; n < a.N; ++n) {
        block_rows_sum<256>(a.ws + (long long)n * a.nblk * L, a.nblk, L, fin);   // barriers inside
        const float* t = fin + 256 * 4;
        for (int o = threadIdx.x; o < L; o += 256) {
            const int c = o / a.nper, k = o % a.nper;
            if (k < 2) a.red[((long long)n * a.C + c) * 2 + k] = t[o];
            tot_n[o] += t[o];
        }
        __syncthreads();
    }
    for (int o = threadIdx.x; o < L; o += 256) {
        const int c = o / a.nper, k = o % a.nper;
        const float tot = tot_n[o];
        if (k == 0) { if (a.dbeta) a.dbeta[c] = a.acc_norm ? a.dbeta[c] + tot : tot; }
        else if (k == 1) { if (a.dgamma) a.dgamma[c] = a.acc_norm ? a.dgamma[c] + tot : tot; }
        else if (k - 2 < a.Cout && a.dw) a.dw[(k - 2) * a.C + c] = a.acc_dw ? a.dw[(k - 2) * a.C + c] + tot : tot;
    }
}

template <typename T, bool DW>
__global__ __launch_bounds__(RED_THREADS) void head_dgrad_inbwd_kernel(const HeadBwdParams p) {
    constexpr int WD = DT<T>::EPC;
    __shared__ float red[RED_THREADS * 2 * WD];
    const int n = blockIdx.y;
    const int g = threadIdx.x % p.groups, rl = threadIdx.x / p.groups;
    const long long r0 = (long long)blockIdx.x * p.rows_per_block;
    long long r1 = r0 + p.rows_per_block;
    if (r1 > p.S) r1 = p.S;
    const T* xn = (const T*)p.x + (long long)n * p.S * p.ldx;
    const T* dyn = (const T*)p.dy + (long long)n * p.S * p.lddy;
    T* dan = (T*)p.da + (long long)n * p.S * p.ldda;
    for (int gbase = 0; gbase * WD < p.C; gbase += p.groups) {   // uniform trip count: barriers inside
        const int gg = gbase + g;
        const bool act = gg * WD < p.C;
        float mean[WD], rstd[WD], sc[WD], sh[WD], a0[WD], a1[WD], wv[4][WD];
        float gw[DW ? 4 : 1][WD];
#pragma unroll
        for (int e = 0; e < WD; ++e) {
            const int c = act ? gg * WD + e : 0;
            mean_rstd(p.stats, n, p.C, c, p.S, p.eps, mean[e], rstd[e]);
            sc[e] = rstd[e] * (p.gamma ? p.gamma[c] : 1.f);
            sh[e] = (p.beta ? p.beta[c] : 0.f) - mean[e] * sc[e];
            a0[e] = a1[e] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) wv[k][e] = k < p.Cout ? (float)(T)p.w[k * p.C + c] : 0.f;
#pragma unroll
            for (int k = 0; k < (DW ? 4 : 1); ++k) gw[k][e] = 0.f;
        }
        if (act && rl < p.rows_par) {
            constexpr int UNR = DW ? 2 : 4;   // the weight-gradient variant carries 32 more accumulators: stay under 256 VGPRs
#pragma unroll UNR
            for (long long r = r0 + rl; r < r1; r += p.rows_par) {
                ChunkV<T> xc, dc, o;
                xc.load(xn + r * p.ldx + gg * WD);
                dc.load(dyn + r * p.lddy);            // the first EPC (>= 4) channels of the class gradient
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const float da = head_da<T, WD>(dc.v, wv, e);
                    o.v[e] = da;
                    const float z = xc.v[e] * sc[e] + sh[e];
                    const float dz = z > 0.f ? da : da * p.slope;
                    a0[e] += dz;
                    a1[e] += dz * ((xc.v[e] - mean[e]) * rstd[e]);
                    if constexpr (DW) {
                        const float av = (float)(T)(z > 0.f ? z : z * p.slope);   // the activation as the forward stored it
#pragma unroll
                        for (int k = 0; k < 4; ++k) gw[k][e] += dc.v[k] * av;
                    }
                }
                // da absent (weight-gradient form only): the apply pass forms it again from dy and w (its HEAD source).  A
                // runtime test, wave-uniform; the form without dW keeps its one code path, and with it its contraction
                if (!DW || p.da != nullptr) o.store(dan + r * p.ldda + gg * WD);
            }
        }
        constexpr int NPER = DW ? 6 : 2;
        float* wsb = p.ws + ((long long)n * gridDim.x + blockIdx.x) * p.C * NPER;
#pragma unroll
        for (int round = 0; round < NPER / 2; ++round) {   // the two-value block reduction, once per value pair
            __syncthreads();
#pragma unroll
            for (int e = 0; e < WD; ++e) {
                float v0, v1;
                if (round == 0) { v0 = a0[e]; v1 = a1[e]; }
                else { v0 = gw[DW ? 2 * round - 2 : 0][e]; v1 = gw[DW ? 2 * round - 1 : 0][e]; }
                red[(threadIdx.x * WD + e) * 2 + 0] = v0;
                red[(threadIdx.x * WD + e) * 2 + 1] = v1;
            }
            __syncthreads();
            block_rows_reduce<WD>(red, p.groups, p.rows_par, g, rl, act);
            if (act && rl == 0) {
                const int kmax = p.rows_par < RED_STAGE2 ? p.rows_par : RED_STAGE2;
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    float a = 0.f, b = 0.f;
                    for (int k = 0; k < kmax; ++k) {
                        a += red[((k * p.groups + g) * WD + e) * 2 + 0];
                        b += red[((k * p.groups + g) * WD + e) * 2 + 1];
                    }
                    wsb[(gg * WD + e) * NPER + 2 * round + 0] = a;
                    wsb[(gg * WD + e) * NPER + 2 * round + 1] = b;
                }
            }
        }
    }
}

// 1x1x1 convolution with a handful of output channels (the segmentation head: 32 -> 2..8 classes).  The implicit-GEMM
// kernels spend a 16-wide MFMA column block on three real outputs; this is a streaming pass instead: one thread per
// voxel reads its Cin channels (16-byte chunks), the weights sit in LDS (same address for every lane: broadcast reads),
// fp32 accumulation, weights rounded to T first so the arithmetic equals the MFMA path's up to summation order.
template <typename T, int COUT>
__global__ __launch_bounds__(256) void conv1x1_head_kernel(const T* __restrict__ x, long long ldx, const float* __restrict__ w,
                                                           const float* __restrict__ bias, T* __restrict__ y, long long ldy,
                                                           long long NV, int Cin) {
    constexpr int WD = DT<T>::EPC;
    __shared__ float wS[COUT * 64];
    for (int i = threadIdx.x; i < COUT * Cin; i += 256) wS[i] = (float)(T)w[i];
    __syncthreads();
    float b[COUT];
#pragma unroll
    for (int c = 0; c < COUT; ++c) b[c] = bias ? bias[c] : 0.f;
    for (long long v = blockIdx.x * 256LL + threadIdx.x; v < NV; v += (long long)gridDim.x * 256) {
        float acc[COUT];
#pragma unroll
        for (int c = 0; c < COUT; ++c) acc[c] = b[c];
        const T* xr = x + v * ldx;
        // the row in pieces of up to four chunks with all loads of a piece issued before the first multiply (a loop of one load
        // per trip kept 16 bytes in flight per thread: 1.7 TB/s on the 48-channel rows of Swin-UNETR's output block)
        for (int k0 = 0; k0 < Cin; k0 += 4 * WD) {
            ChunkV<T> xc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + j * WD < Cin) xc[j].load(xr + k0 + j * WD);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + j * WD < Cin) {
#pragma unroll
                    for (int c = 0; c < COUT; ++c)
#pragma unroll
                        for (int e = 0; e < WD; ++e) acc[c] += xc[j].v[e] * wS[c * Cin + k0 + j * WD + e];
                }
        }
        T* yr = y + v * ldy;
#pragma unroll
        for (int c = 0; c < COUT; ++c) DT<T>::st(yr + c, acc[c]);
    }
}

// The same head reading the RAW conv output of the last conv+norm unit: a = T(lrelu(IN(x))) is formed in registers, so
// the normalised activation of that unit is never written (the backward recomputes it as well, head_dgrad_inbwd_kernel).
template <typename T, int COUT>
__global__ __launch_bounds__(256) void conv1x1_head_norm_kernel(const T* __restrict__ x, long long ldx,
                                                                const float* __restrict__ stats,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float slope, float eps, const float* __restrict__ w,
                                                                const float* __restrict__ bias, T* __restrict__ y,
                                                                long long ldy, long long S, int Cin) {
    constexpr int WD = DT<T>::EPC;
    __shared__ float wS[COUT * 64];
    __shared__ float scS[64], shS[64];
    const int n = blockIdx.y;
    for (int i = threadIdx.x; i < COUT * Cin; i += 256) wS[i] = (float)(T)w[i];
    for (int c = threadIdx.x; c < Cin; c += 256) {
        float mean, rstd;
        mean_rstd(stats, n, Cin, c, S, eps, mean, rstd);
        const float sc = rstd * (gamma ? gamma[c] : 1.f);
        scS[c] = sc;
        shS[c] = (beta ? beta[c] : 0.f) - mean * sc;
    }
    __syncthreads();
    float b[COUT];
#pragma unroll
    for (int c = 0; c < COUT; ++c) b[c] = bias ? bias[c] : 0.f;
    const T* xn = x + (long long)n * S * ldx;
    T* yn = y + (long long)n * S * ldy;
    for (long long v = blockIdx.x * 256LL + threadIdx.x; v < S; v += (long long)gridDim.x * 256) {
        float acc[COUT];
#pragma unroll
        for (int c = 0; c < COUT; ++c) acc[c] = b[c];
        const T* xr = xn + v * ldx;
        // the row in pieces of up to four chunks, all loads of a piece issued before the first use (as conv1x1_head_kernel)
        for (int k0 = 0; k0 < Cin; k0 += 4 * WD) {
            ChunkV<T> xc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + j * WD < Cin) xc[j].load(xr + k0 + j * WD);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + j * WD < Cin) {
#pragma unroll
                    for (int e = 0; e < WD; ++e) {
                        const int k = k0 + j * WD + e;
                        const float z = xc[j].v[e] * scS[k] + shS[k];
                        const float a = (float)(T)(z > 0.f ? z : z * slope);
#pragma unroll
                        for (int c = 0; c < COUT; ++c) acc[c] += a * wS[c * Cin + k];
                    }
                }
        }
        T* yr = yn + v * ldy;
#pragma unroll
        for (int c = 0; c < COUT; ++c) DT<T>::st(yr + c, acc[c]);
    }
}

}  // namespace

extern "C" {

int msseg_conv3d_k1_head_fwd(const void* x, long long ldx, const float* w, const float* bias, void* y, long long ldy,
                             long long NV, int Cin, int Cout, int dtype, msseg_stream_t stream) {
    if (!x || !w || !y || NV < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head: bad args");
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head: bad dtype");
    if (Cout < 1 || Cout > 4 || Cin < 1 || Cin > 64 || !vec_ok(x, ldx, Cin, esz) || ldy < Cout)
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head: needs 1 <= Cout <= 4, Cin <= 64 in 16-byte chunks (got %d -> %d)", Cin, Cout);
    const int g = stream_grid(NV);
#define HEAD(T_, C_) hipLaunchKernelGGL((conv1x1_head_kernel<T_, C_>), dim3(g), dim3(256), 0, (hipStream_t)stream, \
                                        (const T_*)x, ldx, w, bias, (T_*)y, ldy, NV, Cin)
#define HEAD_C(T_) do { if (Cout == 1) HEAD(T_, 1); else if (Cout == 2) HEAD(T_, 2); else if (Cout == 3) HEAD(T_, 3); else HEAD(T_, 4); } while (0)
    for_dtype(dtype, [&](auto t) { HEAD_C(typename decltype(t)::type); });
#undef HEAD_C
#undef HEAD
    MSSEG_CHECK_LAUNCH("conv3d_k1_head");
    return MSSEG_OK;
}

int msseg_conv3d_k1_head_bwd_fused(const void* dy, long long lddy, const float* w, void* da, long long ldda, int N,
                                   long long S, int C, int Cout, const void* yraw, long long ldyraw, const float* fwd_stats,
                                   const float* gamma, const float* beta, float slope, float eps, float* red, float* dgamma,
                                   float* dbeta, int accumulate, float* dw, int dw_accumulate, void* scratch,
                                   size_t scratch_bytes, int dtype, msseg_stream_t stream) {
    if (!dy || !w || (!da && !dw) || !yraw || !fwd_stats || !red || N < 1 || S < 1)   // da == NULL (with dw): da is not stored
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head_bwd_fused: bad args");
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head_bwd_fused: bad dtype");
    if (int rc = scratch_ok(scratch, scratch_bytes, "conv3d_k1_head_bwd_fused")) return rc;
    const int esz = dtype == MSSEG_F32 ? 4 : 2, epc = 16 / esz;
    if (Cout < 1 || Cout > 4 || C < 1 || C > 64 || !vec_ok(yraw, ldyraw, C, esz) || (da && !vec_ok(da, ldda, C, esz)) ||
        (lddy % epc) || ((uintptr_t)dy & 15))
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head_bwd_fused: needs <= 4 classes in 16-byte aligned gradient rows and "
                                 "16-byte channel chunks (C=%d, Cout=%d, lddy=%lld)", C, Cout, lddy);
    HeadBwdParams p{dy, lddy, w, yraw, ldyraw, fwd_stats, gamma, beta, da, ldda, S, C, Cout, eps, slope, 0, 0, 0, nullptr, 0};
    p.ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    p.want_dw = dw != nullptr;
    const int nper = dw ? 6 : 2;
    const RowMap m = row_map(C, epc, RED_THREADS);
    p.groups = m.groups; p.rows_par = m.rows_par;
    long long blocks = reduce_blocks(S, m.rows_par, N, C, nper);
    p.rows_per_block = ceil_div_ll(S, blocks);
    blocks = ceil_div_ll(S, p.rows_per_block);
    dim3 grid((unsigned)blocks, N);
    if (dw) {
        for_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL((head_dgrad_inbwd_kernel<typename decltype(t)::type, true>), grid, dim3(RED_THREADS), 0,
                               (hipStream_t)stream, p);
        });
    } else {
        for_dtype(dtype, [&](auto t) {
            hipLaunchKernelGGL((head_dgrad_inbwd_kernel<typename decltype(t)::type, false>), grid, dim3(RED_THREADS), 0,
                               (hipStream_t)stream, p);
        });
    }
    MSSEG_CHECK_LAUNCH("conv3d_k1_head_dgrad_inbwd");
    HeadFinArgs a{p.ws, N, (int)blocks, C, nper, Cout, red, dbeta, dgamma, dw, accumulate, dw_accumulate};
    hipLaunchKernelGGL(head_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    MSSEG_CHECK_LAUNCH("head_finalize");
    return MSSEG_OK;
}

int msseg_conv3d_k1_head_norm_fwd(const void* x, long long ldx, const float* stats, const float* gamma, const float* beta,
                                  float slope, float eps, const float* w, const float* bias, void* y, long long ldy, int N,
                                  long long S, int Cin, int Cout, int dtype, msseg_stream_t stream) {
    if (!x || !stats || !w || !y || N < 1 || S < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head_norm: bad args");
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head_norm: bad dtype");
    if ((gamma == nullptr) != (beta == nullptr)) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head_norm: gamma/beta go together");
    if (Cout < 1 || Cout > 4 || Cin < 1 || Cin > 64 || !vec_ok(x, ldx, Cin, esz) || ldy < Cout)
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_head_norm: needs 1 <= Cout <= 4, Cin <= 64 in 16-byte chunks (got %d -> %d)", Cin, Cout);
    long long gx = ceil_div_ll(S, 256);
    const long long cap = (long long)msseg_num_cus() * 16 / N + 1;
    if (gx > cap) gx = cap;
    dim3 grid((unsigned)gx, N);
#define HEADN(T_, C_) hipLaunchKernelGGL((conv1x1_head_norm_kernel<T_, C_>), grid, dim3(256), 0, (hipStream_t)stream, \
                                         (const T_*)x, ldx, stats, gamma, beta, slope, eps, w, bias, (T_*)y, ldy, S, Cin)
#define HEADN_C(T_) do { if (Cout == 1) HEADN(T_, 1); else if (Cout == 2) HEADN(T_, 2); else if (Cout == 3) HEADN(T_, 3); else HEADN(T_, 4); } while (0)
    for_dtype(dtype, [&](auto t) { HEADN_C(typename decltype(t)::type); });
#undef HEADN_C
#undef HEADN
    MSSEG_CHECK_LAUNCH("conv3d_k1_head_norm");
    return MSSEG_OK;
}

}  // extern "C"
