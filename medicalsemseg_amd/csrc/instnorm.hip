// InstanceNorm + LeakyReLU (HBM-bound): forward, backward reduce and backward apply, the forward fused with the MaxPool3d(2)
// of an encoder level and its backward counterpart.  Statistics come from channel_reduce.hip or from the convolution that
// produced x; the reductions here end in its second launch (channel_reduce.h).
#include "channel_reduce.h"

#include <initializer_list>

namespace {

// ---------------------------------------------------------------------------------------------------------
// InstanceNorm + LeakyReLU
// ---------------------------------------------------------------------------------------------------------
struct NormParams {
    const void* x; long long ldx;
    const float* stats; const float* gamma; const float* beta;
    const void* res; long long ldr;
    void* y; long long ldy;
    const void* dy; long long lddy;
    float* red;
    void* dx; long long lddx;
    void* dres; long long lddres;
    long long S; int C; float eps, slope;
    long long rows_per_block; int groups, rows_par;
    float* ws; float* dgamma; float* dbeta; int accumulate;
    const float* hw; int hcout;          // MODE 2 with the HEAD source: dy holds the class gradient rows, hw the head's weight
};

// mean_rstd, norm_scale_shift, norm_preact, norm_bwd_dz, norm_bwd_dx: common.h
// MODE 0: forward   MODE 1: backward reduce   MODE 2: backward apply
// (launched for MODE 1, on 16-byte chunks or scalar, and for the scalar fallback of MODE 0 / 2 only: on 16-byte chunks
// those two run instnorm_stream_kernel)
template <typename T, bool VEC, int MODE>
__global__ __launch_bounds__(MODE == 1 ? RED_THREADS : 256) void instnorm_kernel(const NormParams p) {
    static_assert(MODE == 1 || !VEC, "MODE 0 / 2 on 16-byte chunks: instnorm_stream_kernel");
    constexpr int W = VEC ? DT<T>::EPC : 1;
    __shared__ float red[(MODE == 1) ? RED_THREADS * 2 * W : 1];
    const int n = blockIdx.y;
    const int g = threadIdx.x % p.groups, rl = threadIdx.x / p.groups;
    const long long r0 = (long long)blockIdx.x * p.rows_per_block;
    long long r1 = r0 + p.rows_per_block;
    if (r1 > p.S) r1 = p.S;
    const T* xn = (const T*)p.x + (long long)n * p.S * p.ldx;
    const T* yn = (MODE != 0 && p.y != nullptr) ? (const T*)p.y + (long long)n * p.S * p.ldy : nullptr;
    T* yo = (MODE == 0) ? (T*)p.y + (long long)n * p.S * p.ldy : nullptr;
    const T* dyn = (MODE != 0) ? (const T*)p.dy + (long long)n * p.S * p.lddy : nullptr;
    const T* resn = (MODE == 0 && p.res) ? (const T*)p.res + (long long)n * p.S * p.ldr : nullptr;
    T* dxn = (MODE == 2) ? (T*)p.dx + (long long)n * p.S * p.lddx : nullptr;
    T* drn = (MODE == 2 && p.dres) ? (T*)p.dres + (long long)n * p.S * p.lddres : nullptr;
    const float invS = 1.0f / (float)p.S;

    for (int gbase = 0; gbase * W < p.C; gbase += p.groups) {   // uniform trip count: barriers inside
        const int gg = gbase + g;
        const bool act = gg * W < p.C;
        float mean[W], rstd[W], sc[W], sh[W], k0[W], k1[W], a0[W], a1[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const int c = act ? gg * W + e : 0;
            mean_rstd(p.stats, n, p.C, c, p.S, p.eps, mean[e], rstd[e]);
            const float ga = p.gamma ? p.gamma[c] : 1.f;
            sc[e] = rstd[e] * ga;
            sh[e] = (p.beta ? p.beta[c] : 0.f) - mean[e] * sc[e];
            a0[e] = a1[e] = 0.f;
            if constexpr (MODE == 2) {
                k0[e] = p.red[((long long)n * p.C + c) * 2 + 0] * invS;
                k1[e] = p.red[((long long)n * p.C + c) * 2 + 1] * invS;
            }
        }
        if (act && rl < p.rows_par) {
#pragma unroll 4
            for (long long r = r0 + rl; r < r1; r += p.rows_par) {
                float xv[W], o[W], yv[W], dv[W];
                if constexpr (VEC) {
                    ChunkV<T> c; c.load(xn + r * p.ldx + gg * W);
#pragma unroll
                    for (int e = 0; e < W; ++e) xv[e] = c.v[e];
                } else {
                    xv[0] = DT<T>::ld(xn + r * p.ldx + gg);
                }
                if constexpr (MODE == 0) {
                    float rv[W];
#pragma unroll
                    for (int e = 0; e < W; ++e) rv[e] = 0.f;
                    if (resn) {
                        rv[0] = DT<T>::ld(resn + r * p.ldr + gg);
                    }
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        const float z = xv[e] * sc[e] + sh[e] + rv[e];
                        o[e] = z > 0.f ? z : z * p.slope;
                    }
                    DT<T>::st(yo + r * p.ldy + gg, o[0]);
                } else {
                    if constexpr (VEC) {
                        ChunkV<T> d; d.load(dyn + r * p.lddy + gg * W);
#pragma unroll
                        for (int e = 0; e < W; ++e) dv[e] = d.v[e];
                        if (yn != nullptr) {
                            ChunkV<T> c; c.load(yn + r * p.ldy + gg * W);
#pragma unroll
                            for (int e = 0; e < W; ++e) yv[e] = c.v[e];
                        } else {   // sign of the pre-activation, recomputed exactly as the forward formed it
#pragma unroll
                            for (int e = 0; e < W; ++e) yv[e] = xv[e] * sc[e] + sh[e];
                        }
                    } else {
                        dv[0] = DT<T>::ld(dyn + r * p.lddy + gg);
                        yv[0] = (yn != nullptr) ? DT<T>::ld(yn + r * p.ldy + gg) : xv[0] * sc[0] + sh[0];
                    }
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        const float dz = yv[e] > 0.f ? dv[e] : dv[e] * p.slope;
                        const float xh = (xv[e] - mean[e]) * rstd[e];
                        if constexpr (MODE == 1) {
                            a0[e] += dz;
                            a1[e] += dz * xh;
                        } else {
                            o[e] = sc[e] * (dz - k0[e] - xh * k1[e]);
                            dv[e] = dz;
                        }
                    }
                    if constexpr (MODE == 2) {
                        DT<T>::st(dxn + r * p.lddx + gg, o[0]);
                        if (drn) DT<T>::st(drn + r * p.lddres + gg, dv[0]);
                    }
                }
            }
        }
        if constexpr (MODE == 1) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < W; ++e) {
                red[(threadIdx.x * W + e) * 2 + 0] = a0[e];
                red[(threadIdx.x * W + e) * 2 + 1] = a1[e];
            }
            __syncthreads();
            block_rows_reduce<W>(red, p.groups, p.rows_par, g, rl, act);
            if (act && rl == 0) {
                const int kmax = p.rows_par < RED_STAGE2 ? p.rows_par : RED_STAGE2;
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    float a = 0.f, b = 0.f;
                    for (int k = 0; k < kmax; ++k) {
                        a += red[((k * p.groups + g) * W + e) * 2 + 0];
                        b += red[((k * p.groups + g) * W + e) * 2 + 1];
                    }
                    const int c = gg * W + e;
                    float* wsb = p.ws + ((long long)n * gridDim.x + blockIdx.x) * p.C * 2;
                    wsb[c * 2 + 0] = a;
                    wsb[c * 2 + 1] = b;
                }
            }
        }
    }
}

// MODE 0 and MODE 2 on 16-byte chunks are pure streaming passes, elementwise in the rows.  A thread takes NORM_U rows per
// trip: it issues every load of the batch (x, dy, and the residual or the stored activation where the launch has one)
// into registers, then computes, then stores -- no branch stands between the loads, so NORM_U x (1..3) 16-byte loads per
// thread are outstanding at the first wait.  Which optional streams exist is a template parameter (OPT: residual in
// MODE 0, stored activation in MODE 2; DRES: MODE 2 also writes dz).  A tail of fewer than NORM_U rows stays batched: the
// missing rows re-load the trip's first row and their stores are masked.  Rows are addressed by 32-bit byte offsets from
// the block's first row (launch_norm_stream keeps a block's extent below 2^30 bytes in every operand).
// Measured at the UNet's 96^3 x 32 and 48^3 x 64 levels (bf16, batch 2; profiles/README.md): 2 and 4 rows per trip stream
// alike and 8 is slower (backward apply 94-105 against 76 us per call); filling every resident slot (4 to 8 blocks per
// CU) is no faster at 96^3 than 2 blocks per CU and ~5 % slower at 48^3, so the grid stops at NORM_BLOCKS_PER_CU.
constexpr int NORM_U = 4;
constexpr int NORM_BLOCKS_PER_CU = 2;

// one trip: rows rb + u * rows_par, u < NORM_U, of the block's nrows.  TAIL: some of them are past the end (the full trips
// carry no test at all, so that nothing tempts the compiler to move a load behind one)
// HEAD (MODE 2 without OPT / DRES): the incoming gradient is not a tensor.  dyb holds the class gradient rows of the <= 4-class
// head behind this unit (16 bytes per voxel, the same row for every channel chunk) and hwv the head's weights for this chunk:
// dv = head_da(), the value head_dgrad_inbwd_kernel would have stored and this pass read back
template <typename T, int MODE, bool OPT, bool DRES, bool TAIL, bool HEAD = false>
MSSEG_DEVFN void norm_stream_batch(const char* __restrict__ xb, unsigned ldx, const char* __restrict__ ob, unsigned ldo,
                                   const char* __restrict__ dyb, unsigned lddy, char* __restrict__ outb, unsigned ldout,
                                   char* __restrict__ drb, unsigned lddr, int rb, int rows_par, int nrows, unsigned cg,
                                   const float* mean, const float* rstd, const float* sc, const float* sh,
                                   const float* k0, const float* k1, float slope,
                                   const float (*hwv)[DT<T>::EPC] = nullptr) {
    constexpr int W = DT<T>::EPC, U = NORM_U;
    constexpr unsigned ES = sizeof(T);
    unsigned row[U];
    bool ok[U];
    u32x4_t xr[U], dr[U], orw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int r = rb + u * rows_par;
        ok[u] = !TAIL || r < nrows;
        row[u] = (unsigned)(ok[u] ? r : rb);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) xr[u] = ldg16(xb + (row[u] * ldx + cg) * ES);
    if constexpr (MODE == 2) {
#pragma unroll
        for (int u = 0; u < U; ++u) dr[u] = ldg16(dyb + (row[u] * lddy + (HEAD ? 0u : cg)) * ES);
    }
    if constexpr (OPT) {
#pragma unroll
        for (int u = 0; u < U; ++u) orw[u] = ldg16(ob + (row[u] * ldo + cg) * ES);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float xv[W], o[W], dv[W], yv[W];
        Chunk<T>::unpack(xr[u], xv);
        if constexpr (MODE == 0) {
            float rv[W];
            if constexpr (OPT) {
                Chunk<T>::unpack(orw[u], rv);
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) rv[e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float z = xv[e] * sc[e] + sh[e] + rv[e];
                o[e] = z > 0.f ? z : z * slope;
            }
        } else {
            Chunk<T>::unpack(dr[u], dv);
            if constexpr (HEAD) {
                float dl[W];
#pragma unroll
                for (int e = 0; e < W; ++e) dl[e] = dv[e];
#pragma unroll
                for (int e = 0; e < W; ++e) dv[e] = head_da<T, W>(dl, hwv, e);
            }
            if constexpr (OPT) {
                Chunk<T>::unpack(orw[u], yv);
            } else {   // sign of the pre-activation, recomputed exactly as the forward formed it
#pragma unroll
                for (int e = 0; e < W; ++e) yv[e] = norm_preact(xv[e], sc[e], sh[e]);
            }
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const float dz = norm_bwd_dz(yv[e], dv[e], slope);
                o[e] = norm_bwd_dx(xv[e], dz, mean[e], rstd[e], sc[e], k0[e], k1[e]);
                dv[e] = dz;
            }
        }
        if (ok[u]) {
            Chunk<T>::store((T*)(outb + (row[u] * ldout + cg) * ES), o);
            if constexpr (DRES) Chunk<T>::store((T*)(drb + (row[u] * lddr + cg) * ES), dv);
        }
    }
}

template <typename T, int MODE, bool OPT, bool DRES, bool HEAD = false>
__global__ __launch_bounds__(256, HEAD ? NORM_BLOCKS_PER_CU : 4) void instnorm_stream_kernel(const NormParams p) {
    static_assert(MODE == 0 || MODE == 2, "streaming modes only");
    static_assert(!HEAD || (MODE == 2 && !OPT && !DRES), "the head source replaces the gradient tensor of the plain apply");
    constexpr int W = DT<T>::EPC;
    const int n = blockIdx.y;
    const int g = threadIdx.x % p.groups, rl = threadIdx.x / p.groups;
    const long long r0 = (long long)blockIdx.x * p.rows_per_block;
    const long long r1 = r0 + p.rows_per_block > p.S ? p.S : r0 + p.rows_per_block;
    const int nrows = (int)(r1 - r0);
    if (rl >= p.rows_par || rl >= nrows) return;   // no barriers below
    const long long v0 = ((long long)n * p.S + r0) * (long long)sizeof(T);   // the block's first row, in bytes per unit of ld
    const char* xb = (const char*)p.x + v0 * p.ldx;
    const char* ob = nullptr;
    const char* dyb = nullptr;
    char* outb;
    char* drb = nullptr;
    unsigned ldo = 0, lddy = 0, ldout, lddr = 0;
    if constexpr (MODE == 0) {
        if constexpr (OPT) { ob = (const char*)p.res + v0 * p.ldr; ldo = (unsigned)p.ldr; }
        outb = (char*)p.y + v0 * p.ldy; ldout = (unsigned)p.ldy;
    } else {
        if constexpr (OPT) { ob = (const char*)p.y + v0 * p.ldy; ldo = (unsigned)p.ldy; }
        dyb = (const char*)p.dy + v0 * p.lddy; lddy = (unsigned)p.lddy;
        outb = (char*)p.dx + v0 * p.lddx; ldout = (unsigned)p.lddx;
        if constexpr (DRES) { drb = (char*)p.dres + v0 * p.lddres; lddr = (unsigned)p.lddres; }
    }
    const float invS = 1.0f / (float)p.S;
    for (int gg = g; gg * W < p.C; gg += p.groups) {
        float mean[W], rstd[W], sc[W], sh[W], k0[W], k1[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const int c = gg * W + e;
            mean_rstd(p.stats, n, p.C, c, p.S, p.eps, mean[e], rstd[e]);
            norm_scale_shift(p.gamma, p.beta, c, mean[e], rstd[e], sc[e], sh[e]);
            if constexpr (MODE == 2) {
                k0[e] = p.red[((long long)n * p.C + c) * 2 + 0] * invS;
                k1[e] = p.red[((long long)n * p.C + c) * 2 + 1] * invS;
            } else {
                k0[e] = k1[e] = 0.f;
            }
        }
        float hwv[HEAD ? 4 : 1][W];
        if constexpr (HEAD) {   // as head_dgrad_inbwd_kernel sets them up
#pragma unroll
            for (int e = 0; e < W; ++e)
#pragma unroll
                for (int k = 0; k < 4; ++k) hwv[k][e] = k < p.hcout ? (float)(T)p.hw[k * p.C + gg * W + e] : 0.f;
        }
        const unsigned cg = (unsigned)(gg * W);
        int rb = rl;
        for (; rb + (NORM_U - 1) * p.rows_par < nrows; rb += NORM_U * p.rows_par)
            norm_stream_batch<T, MODE, OPT, DRES, false, HEAD>(xb, (unsigned)p.ldx, ob, ldo, dyb, lddy, outb, ldout, drb, lddr, rb,
                                                               p.rows_par, nrows, cg, mean, rstd, sc, sh, k0, k1, p.slope, hwv);
        if (rb < nrows)
            norm_stream_batch<T, MODE, OPT, DRES, true, HEAD>(xb, (unsigned)p.ldx, ob, ldo, dyb, lddy, outb, ldout, drb, lddr, rb,
                                                              p.rows_par, nrows, cg, mean, rstd, sc, sh, k0, k1, p.slope, hwv);
    }
}

// InstanceNorm + LeakyReLU forward fused with the MaxPool3d(2) that follows it in an encoder level: one thread owns a
// 2x2x2 cell x one 16-byte channel chunk, writes the eight activated voxels and their maximum.  The maximum is taken
// over the values as stored (rounded to T), so the pooled tensor equals maxpool2_kernel applied to the stored activation
// bit for bit (same NaN propagation, and the backward's arg-max recomputation sees the same numbers).
struct NormPoolParams {
    const void* x; long long ldx;
    const float* stats; const float* gamma; const float* beta;
    void* y; long long ldy;
    void* pooled; long long ldp;
    int N, D, H, W, C; float eps, slope;
};

template <typename T>
__global__ __launch_bounds__(256) void instnorm_pool_fwd_kernel(const NormPoolParams p) {
    constexpr int WD = DT<T>::EPC;
    const int OD = p.D / 2, OH = p.H / 2, OW = p.W / 2;
    const unsigned ug = (unsigned)(p.C / WD);
    const unsigned total = (unsigned)((long long)p.N * OD * OH * OW * ug);   // < 2^31: checked by the host wrapper
    const long long S = (long long)p.D * p.H * p.W;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        unsigned t = i / ug;
        const int g = (int)(i - t * ug);
        unsigned t2 = t / (unsigned)OW;
        const int ow = (int)(t - t2 * (unsigned)OW);
        t = t2 / (unsigned)OH;
        const int oh = (int)(t2 - t * (unsigned)OH);
        const int n = (int)(t / (unsigned)OD);
        const int od = (int)(t - (unsigned)n * (unsigned)OD);
        float sc[WD], sh[WD], best[WD];
#pragma unroll
        for (int e = 0; e < WD; ++e) {
            const int c = g * WD + e;
            float mean, rstd;
            mean_rstd(p.stats, n, p.C, c, S, p.eps, mean, rstd);
            sc[e] = rstd * (p.gamma ? p.gamma[c] : 1.f);
            sh[e] = (p.beta ? p.beta[c] : 0.f) - mean * sc[e];
            best[e] = -INFINITY;
        }
        ChunkV<T> in[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long vox = (((long long)n * p.D + 2 * od + (k >> 2)) * p.H + 2 * oh + ((k >> 1) & 1)) * p.W + 2 * ow + (k & 1);
            in[k].load((const T*)p.x + vox * p.ldx + g * WD);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long vox = (((long long)n * p.D + 2 * od + (k >> 2)) * p.H + 2 * oh + ((k >> 1) & 1)) * p.W + 2 * ow + (k & 1);
            ChunkV<T> o;
#pragma unroll
            for (int e = 0; e < WD; ++e) {
                const float z = in[k].v[e] * sc[e] + sh[e];
                const float a = (float)(T)(z > 0.f ? z : z * p.slope);
                o.v[e] = a;
                if (a > best[e] || a != a) best[e] = a;
            }
            o.store((T*)p.y + vox * p.ldy + g * WD);
        }
        ChunkV<T> b;
#pragma unroll
        for (int e = 0; e < WD; ++e) b.v[e] = best[e];
        const long long ovox = (((long long)n * OD + od) * OH + oh) * OW + ow;
        b.store((T*)p.pooled + ovox * p.ldp + g * WD);
    }
}

// Backward counterpart for an encoder level: the gradient that reaches the level's activation a = lrelu(IN(x)) is
// skip + maxpool_bwd(a, g) (the decoder's skip gradient plus the pooled path from the level below).  One thread owns a
// 2x2x2 cell x one channel chunk: it recomputes the eight activations from x exactly as the forward stored them (the
// arg-max of the cell, first maximum wins, NaN propagates: maxpool2_kernel's rule), writes
// da = T(skip + [voxel is the arg-max] * g) to a dense tensor and accumulates the InstanceNorm-backward sums
// (sum dz, sum dz * xhat), dz = da * lrelu'(pre-activation) -- what maxpool2_bwd followed by instnorm_kernel<MODE 1> do.
struct NormPoolBwdParams {
    const void* x; long long ldx;
    const float* stats; const float* gamma; const float* beta;
    const void* skip; long long lds;
    const void* g; long long ldg;
    void* da; long long ldda;
    int N, D, H, W, C; float eps, slope;
    int groups, rows_par; long long cells_per_block;
    float* ws;
};

template <typename T>
__global__ __launch_bounds__(RED_THREADS) void instnorm_poolbwd_reduce_kernel(const NormPoolBwdParams p) {
    constexpr int WD = DT<T>::EPC;
    __shared__ float red[RED_THREADS * 2 * WD];
    const int n = blockIdx.y;
    const int g = threadIdx.x % p.groups, rl = threadIdx.x / p.groups;
    const int OD = p.D / 2, OH = p.H / 2, OW = p.W / 2;
    const long long cells = (long long)OD * OH * OW, S = (long long)p.D * p.H * p.W;
    const long long c0 = (long long)blockIdx.x * p.cells_per_block;
    long long c1 = c0 + p.cells_per_block;
    if (c1 > cells) c1 = cells;
    const T* xn = (const T*)p.x + (long long)n * S * p.ldx;
    const T* sn = (const T*)p.skip + (long long)n * S * p.lds;
    const T* gn = (const T*)p.g + (long long)n * cells * p.ldg;
    T* dn = (T*)p.da + (long long)n * S * p.ldda;
    for (int gbase = 0; gbase * WD < p.C; gbase += p.groups) {   // uniform trip count: barriers inside
        const int gg = gbase + g;
        const bool act = gg * WD < p.C;
        float mean[WD], rstd[WD], sc[WD], sh[WD], a0[WD], a1[WD];
#pragma unroll
        for (int e = 0; e < WD; ++e) {
            const int c = act ? gg * WD + e : 0;
            mean_rstd(p.stats, n, p.C, c, S, p.eps, mean[e], rstd[e]);
            sc[e] = rstd[e] * (p.gamma ? p.gamma[c] : 1.f);
            sh[e] = (p.beta ? p.beta[c] : 0.f) - mean[e] * sc[e];
            a0[e] = a1[e] = 0.f;
        }
        if (act && rl < p.rows_par) {
            for (long long cell = c0 + rl; cell < c1; cell += p.rows_par) {
                const int ow = (int)(cell % OW), oh = (int)((cell / OW) % OH), od = (int)(cell / ((long long)OW * OH));
                ChunkV<T> xin[8], gv;
                ChunkV<T> skin[8];
                long long vox[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    vox[k] = ((long long)(2 * od + (k >> 2)) * p.H + 2 * oh + ((k >> 1) & 1)) * p.W + 2 * ow + (k & 1);
                    xin[k].load(xn + vox[k] * p.ldx + gg * WD);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) skin[k].load(sn + vox[k] * p.lds + gg * WD);   // all 17 loads in flight together
                gv.load(gn + cell * p.ldg + gg * WD);
                float best[WD];
                int arg[WD];
#pragma unroll
                for (int e = 0; e < WD; ++e) { best[e] = -INFINITY; arg[e] = 0; }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
#pragma unroll
                    for (int e = 0; e < WD; ++e) {
                        const float z = xin[k].v[e] * sc[e] + sh[e];
                        const float a = (float)(T)(z > 0.f ? z : z * p.slope);
                        if (a > best[e] || a != a) { best[e] = a; arg[e] = k; }
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    ChunkV<T> o;
#pragma unroll
                    for (int e = 0; e < WD; ++e) {
                        const float dv = (float)(T)(skin[k].v[e] + (arg[e] == k ? gv.v[e] : 0.f));
                        o.v[e] = dv;
                        const float z = xin[k].v[e] * sc[e] + sh[e];
                        const float dz = z > 0.f ? dv : dv * p.slope;
                        a0[e] += dz;
                        a1[e] += dz * ((xin[k].v[e] - mean[e]) * rstd[e]);
                    }
                    o.store(dn + vox[k] * p.ldda + gg * WD);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < WD; ++e) {
            red[(threadIdx.x * WD + e) * 2 + 0] = a0[e];
            red[(threadIdx.x * WD + e) * 2 + 1] = a1[e];
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
                float* wsb = p.ws + ((long long)n * gridDim.x + blockIdx.x) * p.C * 2;
                wsb[(gg * WD + e) * 2 + 0] = a;
                wsb[(gg * WD + e) * 2 + 1] = b;
            }
        }
    }
}

// MODE 0 / 2 on 16-byte chunks: one resident set of blocks, sized from what the instantiation really gets per CU
template <typename T, int MODE, bool OPT, bool DRES, bool HEAD = false> int launch_norm_stream(NormParams& p, int N, hipStream_t st) {
    static std::atomic<int> resident{0};   // blocks per CU, asked once per instantiation
    int per_cu = resident.load(std::memory_order_relaxed);
    if (per_cu == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)instnorm_stream_kernel<T, MODE, OPT, DRES, HEAD>,
                                                         256, 0) != hipSuccess || per_cu < 1)
            MSSEG_FAIL(MSSEG_ELAUNCH, "instnorm: no occupancy for the streaming kernel");
        resident.store(per_cu, std::memory_order_relaxed);
    }
    if (per_cu > NORM_BLOCKS_PER_CU) per_cu = NORM_BLOCKS_PER_CU;
    const RowMap m = row_map(p.C, DT<T>::EPC, 256);
    p.groups = m.groups; p.rows_par = m.rows_par;
    // the output is elementwise, so the mapping of rows to blocks is free: every resident block gets one contiguous run of
    // rows, a thread NORM_U rows of it per trip; a run stays below 2^30 bytes in the widest operand (32-bit row offsets)
    long long ldmax = p.ldx > 1 ? p.ldx : 1;
    for (long long ld : {p.ldr, p.ldy, p.lddy, p.lddx, p.lddres}) ldmax = ld > ldmax ? ld : ldmax;
    long long blocks = ceil_div_ll(p.S, (long long)m.rows_par * NORM_U);
    const long long cap = (long long)msseg_num_cus() * per_cu / (N > 0 ? N : 1);
    if (blocks > cap) blocks = cap;
    long long max_run = ((long long)1 << 30) / (ldmax * (long long)sizeof(T)) - 1;   // rows; the chunk offset adds < 1 row
    if (max_run < 1) max_run = 1;
    if (blocks < ceil_div_ll(p.S, max_run)) blocks = ceil_div_ll(p.S, max_run);
    if (blocks < 1) blocks = 1;
    p.rows_per_block = ceil_div_ll(p.S, blocks);
    const long long trip = (long long)m.rows_par * NORM_U;   // whole trips, where the run limit allows: one tail per sample
    if (ceil_div_ll(p.rows_per_block, trip) * trip <= max_run) p.rows_per_block = ceil_div_ll(p.rows_per_block, trip) * trip;
    blocks = ceil_div_ll(p.S, p.rows_per_block);
    hipLaunchKernelGGL((instnorm_stream_kernel<T, MODE, OPT, DRES, HEAD>), dim3((unsigned)blocks, N), dim3(256), 0, st, p);
    MSSEG_CHECK_LAUNCH("instnorm");
    return MSSEG_OK;
}

template <typename T, int MODE> int launch_norm(NormParams& p, int N, bool vec, hipStream_t st) {
    if constexpr (MODE != 1) {
        if (vec) {
            const bool opt = MODE == 0 ? p.res != nullptr : p.y != nullptr;
            if constexpr (MODE == 2) {
                if (p.dres) return opt ? launch_norm_stream<T, 2, true, true>(p, N, st) : launch_norm_stream<T, 2, false, true>(p, N, st);
            }
            return opt ? launch_norm_stream<T, MODE, true, false>(p, N, st) : launch_norm_stream<T, MODE, false, false>(p, N, st);
        }
    }
    constexpr int NTHR = MODE == 1 ? RED_THREADS : 256;
    const RowMap m = row_map(p.C, vec ? DT<T>::EPC : 1, NTHR);
    p.groups = m.groups; p.rows_par = m.rows_par;
    long long blocks;
    if (MODE == 1) {
        blocks = reduce_blocks(p.S, m.rows_par, N, p.C, 2);
    } else {
        // scalar fallback of the streaming modes (channel count or alignment rules out 16-byte chunks)
        blocks = ceil_div_ll(p.S, (long long)m.rows_par * 4);
        const long long cap = (long long)msseg_num_cus() * 8 / (N > 0 ? N : 1);
        if (blocks > cap) blocks = cap;
        if (blocks < 1) blocks = 1;
    }
    p.rows_per_block = ceil_div_ll(p.S, blocks);
    blocks = ceil_div_ll(p.S, p.rows_per_block);
    dim3 grid((unsigned)blocks, N);
    if constexpr (MODE == 1) {
        if (vec) hipLaunchKernelGGL((instnorm_kernel<T, true, 1>), grid, dim3(NTHR), 0, st, p);
        else hipLaunchKernelGGL((instnorm_kernel<T, false, 1>), grid, dim3(NTHR), 0, st, p);
    } else {
        hipLaunchKernelGGL((instnorm_kernel<T, false, MODE>), grid, dim3(NTHR), 0, st, p);
    }
    MSSEG_CHECK_LAUNCH("instnorm");
    if (MODE == 1) {
        // red[n][c] = (sum dz, sum dz*xhat); dbeta = sum_n red0, dgamma = sum_n red1
        return msseg_channels_finalize_launch({p.ws, N, (int)blocks, p.C, 2, 2, p.red, p.dbeta, p.dgamma, p.accumulate}, st);
    }
    return MSSEG_OK;
}

}  // namespace

extern "C" {

int msseg_instnorm_act_fwd(const void* x, long long ldx, const float* stats, const float* gamma, const float* beta,
                           const void* residual, long long ldr, void* y, long long ldy, int N, long long S, int C,
                           float eps, float slope, int dtype, msseg_stream_t stream) {
    if (!x || !stats || !y || N < 1 || S < 1 || C < 1) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_fwd: bad args");
    NormParams p{};
    p.x = x; p.ldx = ldx; p.stats = stats; p.gamma = gamma; p.beta = beta; p.res = residual; p.ldr = ldr;
    p.y = y; p.ldy = ldy; p.S = S; p.C = C; p.eps = eps; p.slope = slope;
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    const bool vec = vec_ok(x, ldx, C, esz) && vec_ok(y, ldy, C, esz) && (!residual || vec_ok(residual, ldr, C, esz));
    int rc = MSSEG_OK;
    const bool known = for_dtype(dtype, [&](auto t) { rc = launch_norm<typename decltype(t)::type, 0>(p, N, vec, (hipStream_t)stream); });
    return known ? rc : bad_dtype(dtype);
}

int msseg_instnorm_act_pool_fwd(const void* x, long long ldx, const float* stats, const float* gamma, const float* beta,
                                void* y, long long ldy, void* pooled, long long ldp, int N, int D, int H, int W, int C,
                                float eps, float slope, int dtype, msseg_stream_t stream) {
    if (!x || !stats || !y || !pooled || N < 1 || D < 2 || H < 2 || W < 2 || C < 1)
        MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_pool_fwd: bad args");
    if ((D | H | W) & 1) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_pool_fwd: odd spatial size %dx%dx%d", D, H, W);
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_pool_fwd: bad dtype");
    if (!(vec_ok(x, ldx, C, esz) && vec_ok(y, ldy, C, esz) && vec_ok(pooled, ldp, C, esz)))
        MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_pool_fwd: needs 16-byte aligned rows and a channel count multiple of %d", 16 / esz);
    const long long total = (long long)N * (D / 2) * (H / 2) * (W / 2) * (C / (16 / esz));
    if (total >= 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_pool_fwd: too many elements");
    NormPoolParams p{x, ldx, stats, gamma, beta, y, ldy, pooled, ldp, N, D, H, W, C, eps, slope};
    for_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(instnorm_pool_fwd_kernel<typename decltype(t)::type>, dim3(stream_grid(total)), dim3(256), 0,
                           (hipStream_t)stream, p);
    });
    MSSEG_CHECK_LAUNCH("instnorm_act_pool_fwd");
    return MSSEG_OK;
}

int msseg_instnorm_act_poolbwd_reduce(const void* x, long long ldx, const float* stats, const float* gamma,
                                      const float* beta, const void* skip, long long lds, const void* g, long long ldg,
                                      void* da, long long ldda, float* red, float* dgamma, float* dbeta, int accumulate,
                                      int N, int D, int H, int W, int C, float eps, float slope, void* scratch,
                                      size_t scratch_bytes, int dtype, msseg_stream_t stream) {
    if (!x || !stats || !skip || !g || !da || !red || N < 1 || D < 2 || H < 2 || W < 2 || C < 1)
        MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_poolbwd_reduce: bad args");
    if ((D | H | W) & 1) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_poolbwd_reduce: odd spatial size %dx%dx%d", D, H, W);
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_poolbwd_reduce: bad dtype");
    if (int rc = scratch_ok(scratch, scratch_bytes, "instnorm_act_poolbwd_reduce")) return rc;
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    if (!(vec_ok(x, ldx, C, esz) && vec_ok(skip, lds, C, esz) && vec_ok(g, ldg, C, esz) && vec_ok(da, ldda, C, esz)))
        MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_poolbwd_reduce: needs 16-byte aligned rows and a channel count multiple of %d",
                   16 / esz);
    NormPoolBwdParams p{x, ldx, stats, gamma, beta, skip, lds, g, ldg, da, ldda, N, D, H, W, C, eps, slope, 0, 0, 0, nullptr};
    p.ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    const RowMap m = row_map(C, 16 / esz, RED_THREADS);
    p.groups = m.groups; p.rows_par = m.rows_par;
    const long long cells = (long long)(D / 2) * (H / 2) * (W / 2);
    // a cell is eight voxel rows of work: one cell per thread while the grid stays within one block per CU
    long long blocks = reduce_blocks(cells * 8, m.rows_par, N, C, 2);
    p.cells_per_block = ceil_div_ll(cells, blocks);
    blocks = ceil_div_ll(cells, p.cells_per_block);
    dim3 grid((unsigned)blocks, N);
    for_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(instnorm_poolbwd_reduce_kernel<typename decltype(t)::type>, grid, dim3(RED_THREADS), 0,
                           (hipStream_t)stream, p);
    });
    MSSEG_CHECK_LAUNCH("instnorm_act_poolbwd_reduce");
    return msseg_channels_finalize_launch({p.ws, N, (int)blocks, C, 2, 2, red, dbeta, dgamma, accumulate}, (hipStream_t)stream);
}

int msseg_instnorm_act_bwd_reduce(const void* x, long long ldx, const float* stats, const float* gamma,
                                  const float* beta, const void* y, long long ldy,
                                  const void* dy, long long lddy, float* red, float* dgamma, float* dbeta,
                                  int accumulate, int N, long long S, int C, float eps, float slope, void* scratch,
                                  size_t scratch_bytes, int dtype, msseg_stream_t stream) {
    if (!x || !stats || !dy || !red) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_bwd_reduce: null pointer");
    if (int rc = scratch_ok(scratch, scratch_bytes, "instnorm_act_bwd_reduce")) return rc;
    NormParams p{};
    p.ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    p.dgamma = dgamma; p.dbeta = dbeta; p.accumulate = accumulate;
    p.x = x; p.ldx = ldx; p.stats = stats; p.gamma = gamma; p.beta = beta; p.y = (void*)y; p.ldy = ldy; p.dy = dy; p.lddy = lddy; p.red = red;
    p.S = S; p.C = C; p.eps = eps; p.slope = slope;
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    const bool vec = vec_ok(x, ldx, C, esz) && vec_ok(y, ldy, C, esz) && vec_ok(dy, lddy, C, esz);
    int rc = MSSEG_OK;
    const bool known = for_dtype(dtype, [&](auto t) { rc = launch_norm<typename decltype(t)::type, 1>(p, N, vec, (hipStream_t)stream); });
    return known ? rc : bad_dtype(dtype);
}

int msseg_instnorm_act_bwd_apply(const void* x, long long ldx, const float* stats, const float* gamma,
                                 const float* beta, const void* y, long long ldy, const void* dy, long long lddy, const float* red, void* dx,
                                 long long lddx, void* dres, long long lddres, int N, long long S, int C, float eps,
                                 float slope, int dtype, msseg_stream_t stream) {
    if (!x || !stats || !dy || !red || !dx) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_bwd_apply: null pointer");
    NormParams p{};
    p.x = x; p.ldx = ldx; p.stats = stats; p.gamma = gamma; p.beta = beta; p.y = (void*)y; p.ldy = ldy; p.dy = dy; p.lddy = lddy;
    p.red = (float*)red; p.dx = dx; p.lddx = lddx; p.dres = dres; p.lddres = lddres;
    p.S = S; p.C = C; p.eps = eps; p.slope = slope;
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    const bool vec = vec_ok(x, ldx, C, esz) && vec_ok(y, ldy, C, esz) && vec_ok(dy, lddy, C, esz) &&
                     vec_ok(dx, lddx, C, esz) && (!dres || vec_ok(dres, lddres, C, esz));
    int rc = MSSEG_OK;
    const bool known = for_dtype(dtype, [&](auto t) { rc = launch_norm<typename decltype(t)::type, 2>(p, N, vec, (hipStream_t)stream); });
    return known ? rc : bad_dtype(dtype);
}

int msseg_instnorm_act_bwd_apply_head(const void* x, long long ldx, const float* stats, const float* gamma,
                                      const float* beta, const void* dl, long long lddl, const float* w, int Cout,
                                      const float* red, void* dx, long long lddx, int N, long long S, int C, float eps,
                                      float slope, int dtype, msseg_stream_t stream) {
    if (!x || !stats || !dl || !w || !red || !dx || N < 1 || S < 1) MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_bwd_apply_head: bad args");
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) return bad_dtype(dtype);
    const int esz = dtype == MSSEG_F32 ? 4 : 2, epc = 16 / esz;
    if (Cout < 1 || Cout > 4 || C < 1 || C > 64 || !vec_ok(x, ldx, C, esz) || !vec_ok(dx, lddx, C, esz) || (lddl % epc) ||
        ((uintptr_t)dl & 15))
        MSSEG_FAIL(MSSEG_EINVAL, "instnorm_act_bwd_apply_head: needs <= 4 classes in 16-byte aligned gradient rows and "
                                 "16-byte channel chunks (C=%d, Cout=%d, lddl=%lld)", C, Cout, lddl);
    NormParams p{};
    p.x = x; p.ldx = ldx; p.stats = stats; p.gamma = gamma; p.beta = beta; p.dy = dl; p.lddy = lddl;
    p.red = (float*)red; p.dx = dx; p.lddx = lddx; p.hw = w; p.hcout = Cout;
    p.S = S; p.C = C; p.eps = eps; p.slope = slope;
    int rc = MSSEG_OK;
    for_dtype(dtype, [&](auto t) { rc = launch_norm_stream<typename decltype(t)::type, 2, false, false, true>(p, N, (hipStream_t)stream); });
    return rc;
}

}  // extern "C"
