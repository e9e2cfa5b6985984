// Pointwise passes (HBM-bound): y = a + b over strided rows, the per-sample scaled residual add of the Swin blocks, GELU.
// 16-byte chunks where the tensors allow them, the scalar form for the rest.
#include "channel_reduce.h"

namespace {

template <typename T>
__global__ void add_kernel(const T* a, long long lda, const T* b, long long ldb, T* y, long long ldy, long long rows,
                           int C) {
    const long long total = rows * C;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long r = i / C;
        DT<T>::st(y + r * ldy + c, DT<T>::ld(a + r * lda + c) + DT<T>::ld(b + r * ldb + c));
    }
}

// the same on 16-byte chunks (rows of C channels inside wider buffers: ld >= C, everything a multiple of a chunk)
template <typename T>
__global__ __launch_bounds__(256) void add_vec_kernel(const T* __restrict__ a, long long lda, const T* __restrict__ b,
                                                      long long ldb, T* __restrict__ y, long long ldy, long long rows, int cpr) {
    constexpr int EPC = DT<T>::EPC;
    const long long total = rows * cpr;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / cpr;
        const int c = (int)(i - r * cpr) * EPC;
        ChunkV<T> ca, cb, o;
        ca.load(a + r * lda + c);
        cb.load(b + r * ldb + c);
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.v[e] = ca.v[e] + cb.v[e];
        o.store(y + r * ldy + c);
    }
}

// y[n][r][:] = a[n][r][:] + s[n] * b[n][r][:]   (a nullable: y = s * b; s nullable: s = 1) -- the residual add of the Swin
// blocks with the per-sample stochastic-depth scale mask[n] / keep folded in (models/layers/drop_path.py:15-45), and its
// backward (branch gradient = s[n] * dy).  16-byte chunks, rows_per_sample rows per sample.
template <typename T>
__global__ __launch_bounds__(256) void axpy_rows_vec_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                            const float* __restrict__ s, T* __restrict__ y,
                                                            long long chunks_per_sample, long long total_chunks) {
    constexpr int EPC = DT<T>::EPC;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total_chunks; i += (long long)gridDim.x * 256) {
        const float sc = s ? s[i / chunks_per_sample] : 1.f;
        ChunkV<T> cb, ca, o;
        cb.load(b + i * EPC);
        if (a) ca.load(a + i * EPC);
#pragma unroll
        for (int e = 0; e < EPC; ++e) o.v[e] = (a ? ca.v[e] : 0.f) + sc * cb.v[e];
        o.store(y + i * EPC);
    }
}

// exact-erf GELU (nn.GELU of the patch merging, swin_nnformer.py:306) and its gradient; 16-byte chunks where the tensors are
// aligned (one element per thread and trip ran at a fraction of the memory rate), the scalar form for the rest
template <typename T, bool BWD>
__global__ void gelu_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out, long long n) {
    constexpr int EPC = DT<T>::EPC;
    const bool vec = ((((uintptr_t)x) | ((uintptr_t)out) | (BWD ? (uintptr_t)dy : 0)) & 15) == 0;
    const long long nvec = vec ? n / EPC : 0;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
        float v[EPC], g[EPC], o[EPC];
        Chunk<T>::load(x + i * EPC, v);
        if constexpr (BWD) Chunk<T>::load(dy + i * EPC, g);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            const float cdf = 0.5f * (1.f + erff(v[e] * 0.70710678118654752f));
            if constexpr (!BWD) o[e] = v[e] * cdf;
            else o[e] = g[e] * (cdf + v[e] * 0.3989422804014327f * expf(-0.5f * v[e] * v[e]));
        }
        Chunk<T>::store(out + i * EPC, o);
    }
    for (long long i = nvec * EPC + blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = DT<T>::ld(x + i);
        const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752f));
        if constexpr (!BWD) DT<T>::st(out + i, v * cdf);
        else DT<T>::st(out + i, DT<T>::ld(dy + i) * (cdf + v * 0.3989422804014327f * expf(-0.5f * v * v)));
    }
}

}  // namespace

extern "C" {

int msseg_add(const void* a, long long lda, const void* b, long long ldb, void* y, long long ldy, long long rows, int C,
              int dtype, msseg_stream_t stream) {
    if (!a || !b || !y || rows < 1 || C < 1) MSSEG_FAIL(MSSEG_EINVAL, "add: bad args");
    {
        const int epc = epc_of(dtype);
        if (C % epc == 0 && lda % epc == 0 && ldb % epc == 0 && ldy % epc == 0 &&
            ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)y)) & 15) == 0) {
            const int cpr = C / epc;
            const int gv = stream_grid(rows * cpr, 512);
            const bool known = for_dtype(dtype, [&](auto t) {
            using T = typename decltype(t)::type;
                hipLaunchKernelGGL(add_vec_kernel<T>, dim3(gv), dim3(256), 0, (hipStream_t)stream, (const T*)a, lda, (const T*)b, ldb,
                                   (T*)y, ldy, rows, cpr);
            });
            if (!known) return bad_dtype(dtype);
            MSSEG_CHECK_LAUNCH("add");
            return MSSEG_OK;
        }
    }
    const int g = stream_grid(rows * C, 1024);
    const bool known = for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(add_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)a, lda, (const T*)b, ldb, (T*)y, ldy,
                           rows, C);
    });
    if (!known) return bad_dtype(dtype);
    MSSEG_CHECK_LAUNCH("add");
    return MSSEG_OK;
}

int msseg_axpy_rows(const void* a, const void* b, const float* scale, void* y, int N, long long elems_per_sample, int dtype,
                    msseg_stream_t stream) {
    if (!b || !y || N < 1 || elems_per_sample < 1) MSSEG_FAIL(MSSEG_EINVAL, "axpy_rows: bad args");
    const int epc = epc_of(dtype);
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "axpy_rows: bad dtype");
    if ((elems_per_sample % epc) || ((uintptr_t)b & 15) || ((uintptr_t)y & 15) || (a && ((uintptr_t)a & 15)))
        MSSEG_FAIL(MSSEG_EINVAL, "axpy_rows: dense 16-byte aligned tensors with elems_per_sample %% %d == 0 expected", epc);
    const long long cps = elems_per_sample / epc, total = cps * N;
    for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(axpy_rows_vec_kernel<T>, dim3(stream_grid(total, 512)), dim3(256), 0, (hipStream_t)stream, (const T*)a,
                           (const T*)b, scale, (T*)y, cps, total);
    });
    MSSEG_CHECK_LAUNCH("axpy_rows");
    return MSSEG_OK;
}

int msseg_gelu_fwd(const void* x, void* y, long long n, int dtype, msseg_stream_t stream) {
    if (!x || !y || n < 1) MSSEG_FAIL(MSSEG_EINVAL, "gelu_fwd: bad args");
    const bool known = for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((gelu_kernel<T, false>), dim3(stream_grid(n, 1024)), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                           (const T*)nullptr, (T*)y, n);
    });
    if (!known) MSSEG_FAIL(MSSEG_EINVAL, "gelu_fwd: bad dtype");
    MSSEG_CHECK_LAUNCH("gelu_fwd");
    return MSSEG_OK;
}

int msseg_gelu_bwd(const void* x, const void* dy, void* dx, long long n, int dtype, msseg_stream_t stream) {
    if (!x || !dy || !dx || n < 1) MSSEG_FAIL(MSSEG_EINVAL, "gelu_bwd: bad args");
    const bool known = for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((gelu_kernel<T, true>), dim3(stream_grid(n, 1024)), dim3(256), 0, (hipStream_t)stream, (const T*)x,
                           (const T*)dy, (T*)dx, n);
    });
    if (!known) MSSEG_FAIL(MSSEG_EINVAL, "gelu_bwd: bad dtype");
    MSSEG_CHECK_LAUNCH("gelu_bwd");
    return MSSEG_OK;
}

}  // extern "C"
