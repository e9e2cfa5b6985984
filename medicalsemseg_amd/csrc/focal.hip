// Streaming kernels of the focal modulation block (models/backbones/focalnet_3d.py:83-106 of the reference) on
// channels-last token volumes, gfx950.  With q | ctx | gates the three channel ranges of ONE Linear output (voxel stride
// ldq / ldg), c1 = GELU(dwconv(ctx)), c2 = GELU(dwconv(c1)):
//
//   spatial sum  : out[n][c] = scale * sum_v x[n][v][c] (* g[n][v]); the per-(sample, channel) mean of c2 with its GELU, and,
//                  weighted by gate 2 and multiplied by gelu'(mean), the gradient that flows back into the mean.  Two
//                  stages with fixed-order sums (deterministic).
//   aggregate    : ctx_all = c1 * g0 + c2 * g1 + GELU(mean)[n][c] * g2 -- and its backward: dc1, dc2 (with the mean's
//                  gradient added), and the three gate gradients, a sum over channels per voxel done by the lanes of one
//                  voxel with a fixed xor tree.
//   product      : y = q * h and its two gradients.
// All bandwidth-bound: 16-byte accesses, every operand read once per pass.
#include "common.h"

namespace {

MSSEG_DEVFN float gelu_cdf(float v) { return 0.5f * (1.f + erff(v * 0.70710678118654752f)); }

// ---- spatial sum -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void focal_sum_kernel(const T* __restrict__ x, long long ldx, const T* __restrict__ g, long long ldg,
                                                        long long S, int C, long long vox_per_block, float* __restrict__ part) {
    constexpr int E = Chunk<T>::E;
    __shared__ float red[256 * E];
    const int nch = C / E, vslots = 256 / nch;
    const int tid = threadIdx.x, ch = tid % nch, vs = tid / nch;
    const int n = blockIdx.y;
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    if (vs < vslots) {
        const long long v0 = (long long)blockIdx.x * vox_per_block;
        long long v1 = v0 + vox_per_block;
        if (v1 > S) v1 = S;
        for (long long v = v0 + vs; v < v1; v += vslots) {
            const long long vox = (long long)n * S + v;
            float f[E];
            Chunk<T>::load(x + vox * ldx + ch * E, f);
            const float gv = g ? DT<T>::ld(g + vox * ldg) : 1.f;
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] = fmaf(f[e], gv, acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) red[tid * E + e] = acc[e];
    __syncthreads();
    if (tid < nch) {
        for (int s = 1; s < vslots; ++s)
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] += red[(s * nch + tid) * E + e];
        float* o = part + ((long long)n * gridDim.x + blockIdx.x) * C + tid * E;
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = acc[e];
    }
}

// mode 0: out0 = scale * sum, out1 = GELU(out0) (if given); mode 1: out0 = scale * sum * gelu'(m_in)
__global__ __launch_bounds__(256) void focal_sum_finalize_kernel(const float* __restrict__ part, int blocks, int NC, int C,
                                                                 const float* __restrict__ m_in, float* __restrict__ out0,
                                                                 float* __restrict__ out1, float scale, int mode) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    const int n = i / C, c = i - n * C;
    float s = 0.f;
    for (int r = 0; r < blocks; ++r) s += part[((long long)n * blocks + r) * C + c];
    s *= scale;
    if (mode == 0) {
        out0[i] = s;
        if (out1) out1[i] = s * gelu_cdf(s);
    } else {
        const float m = m_in[i];
        out0[i] = s * (gelu_cdf(m) + m * 0.3989422804014327f * expf(-0.5f * m * m));
    }
}

// ---- aggregate ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void focal_agg_fwd_kernel(const T* __restrict__ c1, const T* __restrict__ c2,
                                                            const T* __restrict__ gates, long long ldg, const float* __restrict__ gm,
                                                            T* __restrict__ out, long long S, int C, long long total) {
    constexpr int E = Chunk<T>::E;
    const int nch = C / E;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % nch);
        const long long v = i / nch;
        const int n = (int)(v / S);
        const T* gp = gates + v * ldg;
        const float g0 = DT<T>::ld(gp), g1 = DT<T>::ld(gp + 1), g2 = DT<T>::ld(gp + 2);
        float a[E], b[E], o[E];
        Chunk<T>::load(c1 + v * C + ch * E, a);
        Chunk<T>::load(c2 + v * C + ch * E, b);
        const float* m = gm + (long long)n * C + ch * E;
#pragma unroll
        for (int e = 0; e < E; ++e) o[e] = fmaf(m[e], g2, fmaf(b[e], g1, a[e] * g0));
        Chunk<T>::store(out + v * C + ch * E, o);
    }
}

// G lanes (a power of two <= 64) share one voxel and walk its chunks; the three gate gradients are summed over the G lanes
// by an xor tree (fixed order)
template <typename T>
__global__ __launch_bounds__(256) void focal_agg_bwd_kernel(const T* __restrict__ da, const T* __restrict__ c1, const T* __restrict__ c2,
                                                            const T* __restrict__ gates, long long ldg, const float* __restrict__ gm,
                                                            const float* __restrict__ dmv, T* __restrict__ dc1, T* __restrict__ dc2,
                                                            T* __restrict__ dgates, long long lddg, int gate_width, long long S, int C,
                                                            long long NV, int G) {
    constexpr int E = Chunk<T>::E;
    const int nch = C / E;
    const int gl = threadIdx.x & (G - 1);
    const long long vpb = 256 / G;
    for (long long v = (long long)blockIdx.x * vpb + threadIdx.x / G; v < NV; v += (long long)gridDim.x * vpb) {
        const int n = (int)(v / S);
        const T* gp = gates + v * ldg;
        const float g0 = DT<T>::ld(gp), g1 = DT<T>::ld(gp + 1);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int ch = gl; ch < nch; ch += G) {
            float d[E], a[E], b[E], o1[E], o2[E];
            const long long off = v * C + ch * E;
            Chunk<T>::load(da + off, d);
            Chunk<T>::load(c1 + off, a);
            Chunk<T>::load(c2 + off, b);
            const float* m = gm + (long long)n * C + ch * E;
            const float* dm = dmv + (long long)n * C + ch * E;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                o1[e] = d[e] * g0;
                o2[e] = fmaf(d[e], g1, dm[e]);
                s0 = fmaf(d[e], a[e], s0);
                s1 = fmaf(d[e], b[e], s1);
                s2 = fmaf(d[e], m[e], s2);
            }
            Chunk<T>::store(dc1 + off, o1);
            Chunk<T>::store(dc2 + off, o2);
        }
        for (int o = G >> 1; o > 0; o >>= 1) {
            s0 += __shfl_xor(s0, o);
            s1 += __shfl_xor(s1, o);
            s2 += __shfl_xor(s2, o);
        }
        if (gl == 0) {
            T* o = dgates + v * lddg;
            DT<T>::st(o, s0); DT<T>::st(o + 1, s1); DT<T>::st(o + 2, s2);
            for (int k = 3; k < gate_width; ++k) DT<T>::st(o + k, 0.f);
        }
    }
}

// ---- product -----------------------------------------------------------------------------------------------------
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void focal_mul_kernel(const T* __restrict__ a, const T* __restrict__ q, long long ldq,
                                                        const T* __restrict__ h, T* __restrict__ o0, long long ldo0, T* __restrict__ o1,
                                                        int C, long long total) {
    // forward: o0[v] = q[v] * h[v] (a unused, ldo0 = C).  backward: a = dy, o0 = dq (stride ldo0) = dy * h, o1 = dh = dy * q
    constexpr int E = Chunk<T>::E;
    const int nch = C / E;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % nch);
        const long long v = i / nch;
        float qf[E], hf[E], r0[E];
        Chunk<T>::load(q + v * ldq + ch * E, qf);
        Chunk<T>::load(h + v * C + ch * E, hf);
        if constexpr (!BWD) {
#pragma unroll
            for (int e = 0; e < E; ++e) r0[e] = qf[e] * hf[e];
            Chunk<T>::store(o0 + v * ldo0 + ch * E, r0);
        } else {
            float df[E], r1[E];
            Chunk<T>::load(a + v * C + ch * E, df);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                r0[e] = df[e] * hf[e];
                r1[e] = df[e] * qf[e];
            }
            Chunk<T>::store(o0 + v * ldo0 + ch * E, r0);
            Chunk<T>::store(o1 + v * C + ch * E, r1);
        }
    }
}

int chk(int dtype, int C, const char* what) {
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "%s: bad dtype", what);
    const int epc = epc_of(dtype);
    if (C < 1 || C % epc) MSSEG_FAIL(MSSEG_EINVAL, "%s: channels must be a multiple of %d", what, epc);
    return MSSEG_OK;
}

bool al16(const void* p) { return p && !((uintptr_t)p & 15); }

}  // namespace

extern "C" {

int msseg_focal_spatial_sum(const void* x, long long ldx, const void* g, long long ldg, const float* m_in, float* out0, float* out1,
                            float scale, int mode, int N, long long S, int C, void* scratch, size_t scratch_bytes, int dtype,
                            msseg_stream_t stream) {
    if (int rc = chk(dtype, C, "focal_spatial_sum")) return rc;
    const int epc = epc_of(dtype);
    if (!al16(x) || !out0 || N < 1 || S < 1 || ldx < C || ldx % epc || C / epc > 256 || (mode != 0 && mode != 1) ||
        (mode == 1 && !m_in) || (g && ldg < 1))
        MSSEG_FAIL(MSSEG_EINVAL, "focal_spatial_sum: bad args");
    if (int rc = scratch_ok(scratch, scratch_bytes, "focal_spatial_sum")) return rc;
    float* part = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    const int vslots = 256 / (C / epc);
    long long blocks = ceil_div_ll(S, (long long)vslots * 8);
    const long long cap = (long long)msseg_num_cus() * 4 / N + 1;
    if (blocks > cap) blocks = cap;
    const long long fit = (long long)((scratch_bytes - MSSEG_SCRATCH_HEADER_BYTES) / ((size_t)N * C * sizeof(float)));
    if (blocks > fit) blocks = fit;
    if (blocks < 1) MSSEG_FAIL(MSSEG_EINVAL, "focal_spatial_sum: %d x %d channels exceed the reduce scratch", N, C);
    const long long vpb = ceil_div_ll(S, blocks);
    blocks = ceil_div_ll(S, vpb);
    hipStream_t s = (hipStream_t)stream;
    for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(focal_sum_kernel<T>, dim3((unsigned)blocks, N), dim3(256), 0, s, (const T*)x, ldx, (const T*)g, ldg, S, C,
                           vpb, part);
    });
    MSSEG_CHECK_LAUNCH("focal_spatial_sum");
    hipLaunchKernelGGL(focal_sum_finalize_kernel, dim3(ceil_div(N * C, 256)), dim3(256), 0, s, part, (int)blocks, N * C, C, m_in, out0,
                       out1, scale, mode);
    MSSEG_CHECK_LAUNCH("focal_spatial_sum_finalize");
    return MSSEG_OK;
}

int msseg_focal_aggregate_fwd(const void* c1, const void* c2, const void* gates, long long ldg, const float* gm, void* out, int N,
                              long long S, int C, int dtype, msseg_stream_t stream) {
    if (int rc = chk(dtype, C, "focal_aggregate_fwd")) return rc;
    if (!al16(c1) || !al16(c2) || !al16(out) || !gates || !gm || N < 1 || S < 1 || ldg < 3)
        MSSEG_FAIL(MSSEG_EINVAL, "focal_aggregate_fwd: bad args");
    const long long total = (long long)N * S * (C / epc_of(dtype));
    for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(focal_agg_fwd_kernel<T>, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, (const T*)c1,
                           (const T*)c2, (const T*)gates, ldg, gm, (T*)out, S, C, total);
    });
    MSSEG_CHECK_LAUNCH("focal_aggregate_fwd");
    return MSSEG_OK;
}

int msseg_focal_aggregate_bwd(const void* da, const void* c1, const void* c2, const void* gates, long long ldg, const float* gm,
                              const float* dmv, void* dc1, void* dc2, void* dgates, long long lddg, int gate_width, int N,
                              long long S, int C, int dtype, msseg_stream_t stream) {
    if (int rc = chk(dtype, C, "focal_aggregate_bwd")) return rc;
    if (!al16(da) || !al16(c1) || !al16(c2) || !al16(dc1) || !al16(dc2) || !gates || !gm || !dmv || !dgates || N < 1 || S < 1 ||
        ldg < 3 || gate_width < 3 || lddg < gate_width)
        MSSEG_FAIL(MSSEG_EINVAL, "focal_aggregate_bwd: bad args");
    const int nch = C / epc_of(dtype);
    int G = 1;
    while (G < nch && G < 64) G <<= 1;
    const long long NV = (long long)N * S;
    for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(focal_agg_bwd_kernel<T>, dim3(stream_grid(NV * G)), dim3(256), 0, (hipStream_t)stream, (const T*)da,
                           (const T*)c1, (const T*)c2, (const T*)gates, ldg, gm, dmv, (T*)dc1, (T*)dc2, (T*)dgates, lddg, gate_width,
                           S, C, NV, G);
    });
    MSSEG_CHECK_LAUNCH("focal_aggregate_bwd");
    return MSSEG_OK;
}

int msseg_focal_mul_fwd(const void* q, long long ldq, const void* h, void* y, long long rows, int C, int dtype,
                        msseg_stream_t stream) {
    if (int rc = chk(dtype, C, "focal_mul_fwd")) return rc;
    const int epc = epc_of(dtype);
    if (!al16(q) || !al16(h) || !al16(y) || rows < 1 || ldq < C || ldq % epc) MSSEG_FAIL(MSSEG_EINVAL, "focal_mul_fwd: bad args");
    const long long total = rows * (C / epc);
    for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((focal_mul_kernel<T, false>), dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream,
                           (const T*)nullptr, (const T*)q, ldq, (const T*)h, (T*)y, (long long)C, (T*)nullptr, C, total);
    });
    MSSEG_CHECK_LAUNCH("focal_mul_fwd");
    return MSSEG_OK;
}

int msseg_focal_mul_bwd(const void* dy, const void* q, long long ldq, const void* h, void* dq, long long lddq, void* dh,
                        long long rows, int C, int dtype, msseg_stream_t stream) {
    if (int rc = chk(dtype, C, "focal_mul_bwd")) return rc;
    const int epc = epc_of(dtype);
    if (!al16(dy) || !al16(q) || !al16(h) || !al16(dq) || !al16(dh) || rows < 1 || ldq < C || ldq % epc || lddq < C || lddq % epc)
        MSSEG_FAIL(MSSEG_EINVAL, "focal_mul_bwd: bad args");
    const long long total = rows * (C / epc);
    for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((focal_mul_kernel<T, true>), dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, (const T*)dy,
                           (const T*)q, ldq, (const T*)h, (T*)dq, lddq, (T*)dh, C, total);
    });
    MSSEG_CHECK_LAUNCH("focal_mul_bwd");
    return MSSEG_OK;
}

}  // extern "C"
