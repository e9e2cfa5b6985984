// LayerNorm over channels (HBM-bound): forward, backward, backward with a residual gradient added, and the parameter
// gradient, whose reduction ends in the second launch of channel_reduce.h.
#include "channel_reduce.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// LayerNorm over channels (one thread per token)
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const T* __restrict__ x, long long ldx, const float* g,
                                                            const float* bta, T* __restrict__ y, long long ldy,
                                                            float* mean, float* rstd, long long rows, int C, float eps) {
    for (long long r = blockIdx.x * 256LL + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
        const T* xr = x + r * ldx;
        float s = 0.f, s2 = 0.f;
        for (int c = 0; c < C; ++c) { const float v = DT<T>::ld(xr + c); s += v; s2 += v * v; }
        const float mu = s / C;
        float var = s2 / C - mu * mu;
        var = var > 0.f ? var : 0.f;
        const float rs = rsqrtf(var + eps);
        if (mean) { mean[r] = mu; rstd[r] = rs; }
        T* yr = y + r * ldy;
        for (int c = 0; c < C; ++c)
            DT<T>::st(yr + c, (DT<T>::ld(xr + c) - mu) * rs * (g ? g[c] : 1.f) + (bta ? bta[c] : 0.f));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const T* __restrict__ x, long long ldx, const float* g,
                                                            const float* mean, const float* rstd,
                                                            const T* __restrict__ dy, long long lddy, T* __restrict__ dx,
                                                            long long lddx, float* dg, float* db, long long rows, int C) {
    for (long long r = blockIdx.x * 256LL + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
        const T* xr = x + r * ldx;
        const T* dr = dy + r * lddy;
        const float mu = mean[r], rs = rstd[r];
        float a = 0.f, b = 0.f;
        for (int c = 0; c < C; ++c) {
            const float dyg = DT<T>::ld(dr + c) * (g ? g[c] : 1.f);
            const float xh = (DT<T>::ld(xr + c) - mu) * rs;
            a += dyg; b += dyg * xh;
        }
        a /= C; b /= C;
        T* dxr = dx + r * lddx;
        for (int c = 0; c < C; ++c) {
            const float d = DT<T>::ld(dr + c);
            const float xh = (DT<T>::ld(xr + c) - mu) * rs;
            DT<T>::st(dxr + c, rs * (d * (g ? g[c] : 1.f) - a - xh * b));
        }
    }
}

// Vector forms: LPR lanes (a power of two <= 64) share one token row, 16-byte chunks, the row stays in registers between
// the statistics and the normalisation (one pass over HBM); reductions by xor-shuffles inside the lane group.
struct LnVecParams {
    const void* x; long long ldx; const float* g; const float* b; void* y; long long ldy;
    float* mean; float* rstd; const void* dy; long long lddy; long long rows; int C, lpr, nch; float eps;
    const void* add; long long ldadd;   // backward: dx = T(layernorm backward) + add (the gradient of a residual branch that left x)
};

template <typename T, int MAXCH, bool BWD>
__global__ __launch_bounds__(256) void layernorm_vec_kernel(const LnVecParams p) {
    constexpr int EPC = DT<T>::EPC;
    const int lane = threadIdx.x & 63, sub = lane & (p.lpr - 1), rows_per_wave = 64 / p.lpr;
    const long long wave_id = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * 4;
    const float invC = 1.0f / (float)p.C;
    // per-chunk affine parameters of this lane
    float gv[MAXCH][EPC], bv[MAXCH][EPC];
#pragma unroll
    for (int k = 0; k < MAXCH; ++k) {
        const int ch = sub + k * p.lpr;
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            gv[k][e] = (ch < p.nch && p.g) ? p.g[ch * EPC + e] : 1.f;
            bv[k][e] = (!BWD && ch < p.nch && p.b) ? p.b[ch * EPC + e] : 0.f;
        }
    }
    for (long long r0 = wave_id * rows_per_wave; r0 < p.rows; r0 += nwaves * rows_per_wave) {
        const long long r = r0 + lane / p.lpr;
        const bool rok = r < p.rows;
        float xv[MAXCH][EPC], dv[MAXCH][EPC];
#pragma unroll
        for (int k = 0; k < MAXCH; ++k) {
            const int ch = sub + k * p.lpr;
            const bool ok = rok && ch < p.nch;
#pragma unroll
            for (int e = 0; e < EPC; ++e) xv[k][e] = dv[k][e] = 0.f;
            if (ok) {
                Chunk<T>::load((const T*)p.x + r * p.ldx + ch * EPC, xv[k]);
                if constexpr (BWD) Chunk<T>::load((const T*)p.dy + r * p.lddy + ch * EPC, dv[k]);
            }
        }
        if constexpr (!BWD) {
            // the row is in registers: mean first, then the centred sum of squares (E[x^2] - mean^2 loses
            // eps * mean^2 / var, which shows on wide rows with a large mean)
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < MAXCH; ++k)
#pragma unroll
                for (int e = 0; e < EPC; ++e) s += xv[k][e];
            for (int o = p.lpr >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
            const float mu = s * invC;
            float s2 = 0.f;
#pragma unroll
            for (int k = 0; k < MAXCH; ++k) {
                if (sub + k * p.lpr < p.nch) {
#pragma unroll
                    for (int e = 0; e < EPC; ++e) { const float d = xv[k][e] - mu; s2 += d * d; }
                }
            }
            for (int o = p.lpr >> 1; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
            const float var = s2 * invC;
            const float rs = rsqrtf(var + p.eps);
            if (rok && sub == 0 && p.mean) { p.mean[r] = mu; p.rstd[r] = rs; }
#pragma unroll
            for (int k = 0; k < MAXCH; ++k) {
                const int ch = sub + k * p.lpr;
                if (rok && ch < p.nch) {
                    float o[EPC];
#pragma unroll
                    for (int e = 0; e < EPC; ++e) o[e] = (xv[k][e] - mu) * rs * gv[k][e] + bv[k][e];
                    Chunk<T>::store((T*)p.y + r * p.ldy + ch * EPC, o);
                }
            }
        } else {
            const float mu = rok ? p.mean[r] : 0.f, rs = rok ? p.rstd[r] : 0.f;
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int k = 0; k < MAXCH; ++k)
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const float dyg = dv[k][e] * gv[k][e];
                    a += dyg;
                    b += dyg * ((xv[k][e] - mu) * rs);
                }
            for (int o = p.lpr >> 1; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
            a *= invC; b *= invC;
#pragma unroll
            for (int k = 0; k < MAXCH; ++k) {
                const int ch = sub + k * p.lpr;
                if (rok && ch < p.nch) {
                    float o[EPC];
#pragma unroll
                    for (int e = 0; e < EPC; ++e) o[e] = rs * (dv[k][e] * gv[k][e] - a - (xv[k][e] - mu) * rs * b);
                    if (p.add) {   // the sum autograd forms for a tensor with two consumers: both terms rounded to T, then added
                        float r2[EPC];
                        Chunk<T>::load((const T*)p.add + r * p.ldadd + ch * EPC, r2);
#pragma unroll
                        for (int e = 0; e < EPC; ++e) o[e] = (float)(T)o[e] + r2[e];
                    }
                    Chunk<T>::store((T*)p.y + r * p.ldy + ch * EPC, o);
                }
            }
        }
    }
}

// returns false when the vector form does not apply (unaligned rows / odd channel counts)
template <typename T, bool BWD> bool launch_ln_vec(LnVecParams p, hipStream_t stream) {
    constexpr int EPC = DT<T>::EPC;
    const size_t esz = sizeof(T);
    if (p.C % EPC || ((uintptr_t)p.x & 15) || ((uintptr_t)p.y & 15) || (p.ldx * esz) % 16 || (p.ldy * esz) % 16) return false;
    if (BWD && (((uintptr_t)p.dy & 15) || (p.lddy * esz) % 16)) return false;
    p.nch = p.C / EPC;
    int lpr = 1;
    while (lpr < p.nch && lpr < 64) lpr <<= 1;
    p.lpr = lpr;
    const int maxch = (p.nch + lpr - 1) / lpr;
    // (rows wider than 8 x 64 chunks -- 4096 bf16 channels -- fall back to the scalar kernel: one thread per row.  The 3072-wide
    //  LayerNorm of the MONAI variant's last patch merging ran there at 1 ms per pass for 54 rows.)
    if (maxch > 8) return false;
    const long long waves = (p.rows + (64 / lpr) - 1) / (64 / lpr);
    long long blocks = (waves + 3) / 4;
    const long long cap = (long long)msseg_num_cus() * 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    dim3 grid((unsigned)blocks);
    switch (maxch) {
        case 1: hipLaunchKernelGGL((layernorm_vec_kernel<T, 1, BWD>), grid, dim3(256), 0, stream, p); break;
        case 2: hipLaunchKernelGGL((layernorm_vec_kernel<T, 2, BWD>), grid, dim3(256), 0, stream, p); break;
        case 3: hipLaunchKernelGGL((layernorm_vec_kernel<T, 3, BWD>), grid, dim3(256), 0, stream, p); break;
        case 4: hipLaunchKernelGGL((layernorm_vec_kernel<T, 4, BWD>), grid, dim3(256), 0, stream, p); break;
        case 5: case 6: hipLaunchKernelGGL((layernorm_vec_kernel<T, 6, BWD>), grid, dim3(256), 0, stream, p); break;
        default: hipLaunchKernelGGL((layernorm_vec_kernel<T, 8, BWD>), grid, dim3(256), 0, stream, p); break;
    }
    return true;
}

// LayerNorm parameter gradients: dgamma[c] = sum_rows dy*xhat, dbeta[c] = sum_rows dy  (xhat from per-row mean/rstd)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void ln_param_grad_kernel(const T* __restrict__ x, long long ldx,
                                                            const T* __restrict__ dy, long long lddy,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            long long rows, int C, int groups, int rows_par,
                                                            long long rows_per_block, float* ws,
                                                            float* dgamma, float* dbeta, int accumulate) {
    constexpr int W = VEC ? DT<T>::EPC : 1;
    __shared__ float red[256 * 2 * (VEC ? DT<T>::EPC : 1)];
    const int g = threadIdx.x % groups, rl = threadIdx.x / groups;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    long long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    float* wsb = ws + (long long)blockIdx.x * C * 2;
    for (int gbase = 0; gbase * W < C; gbase += groups) {
        const int gg = gbase + g;
        const bool act = gg * W < C;
        float s[W], s2[W];
#pragma unroll
        for (int e = 0; e < W; ++e) s[e] = s2[e] = 0.f;
        if (act && rl < rows_par) {
#pragma unroll 4
            for (long long r = r0 + rl; r < r1; r += rows_par) {
                const float mu = mean[r], rs = rstd[r];
                if constexpr (VEC) {
                    ChunkV<T> cx, cd;
                    cx.load(x + r * ldx + gg * W);
                    cd.load(dy + r * lddy + gg * W);
#pragma unroll
                    for (int e = 0; e < W; ++e) { s[e] += cd.v[e] * (cx.v[e] - mu) * rs; s2[e] += cd.v[e]; }
                } else {
                    const float d = DT<T>::ld(dy + r * lddy + gg);
                    s[0] += d * (DT<T>::ld(x + r * ldx + gg) - mu) * rs;
                    s2[0] += d;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < W; ++e) {
            red[(threadIdx.x * W + e) * 2 + 0] = s[e];
            red[(threadIdx.x * W + e) * 2 + 1] = s2[e];
        }
        __syncthreads();
        if (act && rl == 0) {
#pragma unroll
            for (int e = 0; e < W; ++e) {
                float a = 0.f, b = 0.f;
                for (int k = 0; k < rows_par; ++k) {
                    a += red[((k * groups + g) * W + e) * 2 + 0];
                    b += red[((k * groups + g) * W + e) * 2 + 1];
                }
                wsb[(gg * W + e) * 2 + 0] = a;
                wsb[(gg * W + e) * 2 + 1] = b;
            }
        }
    }
}

template <typename T>
int launch_ln_param_grad(const void* x, long long ldx, const void* dy, long long lddy, const float* mean, const float* rstd,
                         float* dgamma, float* dbeta, int accumulate, long long rows, int C, void* scratch, hipStream_t st) {
    const bool vec = vec_ok(x, ldx, C, sizeof(T)) && vec_ok(dy, lddy, C, sizeof(T));
    const RowMap m = row_map(C, vec ? DT<T>::EPC : 1);
    long long blocks = reduce_blocks(rows, m.rows_par, 1, C, 2);
    const long long rpb = ceil_div_ll(rows, blocks);
    blocks = ceil_div_ll(rows, rpb);
    float* ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    if (vec)
        hipLaunchKernelGGL((ln_param_grad_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, ldx,
                           (const T*)dy, lddy, mean, rstd, rows, C, m.groups, m.rows_par, rpb, ws, dgamma, dbeta, accumulate);
    else
        hipLaunchKernelGGL((ln_param_grad_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, ldx,
                           (const T*)dy, lddy, mean, rstd, rows, C, m.groups, m.rows_par, rpb, ws, dgamma, dbeta, accumulate);
    MSSEG_CHECK_LAUNCH("ln_param_grad");
    return msseg_channels_finalize_launch({ws, 1, (int)blocks, C, 2, 2, ws + blocks * C * 2, dgamma, dbeta, accumulate}, st);
}

}  // namespace

extern "C" {

int msseg_layernorm_fwd(const void* x, long long ldx, const float* gamma, const float* beta, void* y, long long ldy,
                        float* mean, float* rstd, long long rows, int C, float eps, int dtype, msseg_stream_t stream) {
    if (!x || !y || rows < 1 || C < 1) MSSEG_FAIL(MSSEG_EINVAL, "layernorm_fwd: bad args");
    LnVecParams v{};
    v.x = x; v.ldx = ldx; v.g = gamma; v.b = beta; v.y = y; v.ldy = ldy; v.mean = mean; v.rstd = rstd;
    v.rows = rows; v.C = C; v.eps = eps;
    bool done = false;   // by the vector kernel
    for_dtype(dtype, [&](auto t) { done = launch_ln_vec<typename decltype(t)::type, false>(v, (hipStream_t)stream); });
    const bool known = done || for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(layernorm_fwd_kernel<T>, dim3(stream_grid(rows)), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx,
                           gamma, beta, (T*)y, ldy, mean, rstd, rows, C, eps);
    });
    if (!known) MSSEG_FAIL(MSSEG_EINVAL, "layernorm_fwd: bad dtype");
    MSSEG_CHECK_LAUNCH("layernorm_fwd");
    return MSSEG_OK;
}

int msseg_layernorm_bwd(const void* x, long long ldx, const float* gamma, const float* mean, const float* rstd,
                        const void* dy, long long lddy, void* dx, long long lddx, long long rows, int C, int dtype,
                        msseg_stream_t stream) {
    if (!x || !mean || !rstd || !dy || !dx || rows < 1 || C < 1) MSSEG_FAIL(MSSEG_EINVAL, "layernorm_bwd: bad args");
    LnVecParams v{};
    v.x = x; v.ldx = ldx; v.g = gamma; v.y = dx; v.ldy = lddx; v.mean = (float*)mean; v.rstd = (float*)rstd;
    v.dy = dy; v.lddy = lddy; v.rows = rows; v.C = C;
    float* dgamma = nullptr;
    float* dbeta = nullptr;
    bool done = false;   // by the vector kernel
    for_dtype(dtype, [&](auto t) { done = launch_ln_vec<typename decltype(t)::type, true>(v, (hipStream_t)stream); });
    const bool known = done || for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(layernorm_bwd_kernel<T>, dim3(stream_grid(rows)), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx,
                           gamma, mean, rstd, (const T*)dy, lddy, (T*)dx, lddx, dgamma, dbeta, rows, C);
    });
    if (!known) MSSEG_FAIL(MSSEG_EINVAL, "layernorm_bwd: bad dtype");
    MSSEG_CHECK_LAUNCH("layernorm_bwd");
    return MSSEG_OK;
}

int msseg_layernorm_bwd_add(const void* x, long long ldx, const float* gamma, const float* mean, const float* rstd,
                            const void* dy, long long lddy, const void* add, long long ldadd, void* dx, long long lddx,
                            long long rows, int C, int dtype, msseg_stream_t stream) {
    if (!x || !mean || !rstd || !dy || !dx || !add || rows < 1 || C < 1) MSSEG_FAIL(MSSEG_EINVAL, "layernorm_bwd_add: bad args");
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "layernorm_bwd_add: bad dtype");
    const size_t esz = dtype == MSSEG_F32 ? 4 : 2;
    if (((uintptr_t)add & 15) || (ldadd * esz) % 16) MSSEG_FAIL(MSSEG_EINVAL, "layernorm_bwd_add: `add` must have 16-byte aligned rows");
    LnVecParams v{};
    v.x = x; v.ldx = ldx; v.g = gamma; v.y = dx; v.ldy = lddx; v.mean = (float*)mean; v.rstd = (float*)rstd;
    v.dy = dy; v.lddy = lddy; v.rows = rows; v.C = C; v.add = add; v.ldadd = ldadd;
    bool done = false;
    for_dtype(dtype, [&](auto t) { done = launch_ln_vec<typename decltype(t)::type, true>(v, (hipStream_t)stream); });
    if (!done) MSSEG_FAIL(MSSEG_EINVAL, "layernorm_bwd_add: rows of %d channels do not take the vector kernel (16-byte chunks, <= 4096 channels)", C);
    MSSEG_CHECK_LAUNCH("layernorm_bwd_add");
    return MSSEG_OK;
}

int msseg_layernorm_param_grad(const void* x, long long ldx, const float* mean, const float* rstd, const void* dy,
                               long long lddy, float* dgamma, float* dbeta, int accumulate, long long rows, int C,
                               void* scratch, size_t scratch_bytes, int dtype, msseg_stream_t stream) {
    if (!x || !mean || !rstd || !dy || !dgamma || !dbeta || rows < 1 || C < 1)
        MSSEG_FAIL(MSSEG_EINVAL, "layernorm_param_grad: bad args");
    if (int rc = scratch_ok(scratch, scratch_bytes, "layernorm_param_grad")) return rc;
    int rc = MSSEG_OK;
    const bool known = for_dtype(dtype, [&](auto t) {
        rc = launch_ln_param_grad<typename decltype(t)::type>(x, ldx, dy, lddy, mean, rstd, dgamma, dbeta, accumulate, rows, C, scratch,
                                                              (hipStream_t)stream);
    });
    return known ? rc : bad_dtype(dtype);
}

}  // extern "C"
