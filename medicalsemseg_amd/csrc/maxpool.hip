// MaxPool3d(2), forward and backward (HBM-bound).  Channels-last with an explicit voxel stride; 16-byte vector accesses when
// the channel count allows, scalar fallback otherwise.
#include "channel_reduce.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// MaxPool3d(2)
// ---------------------------------------------------------------------------------------------------------
template <typename T, bool VEC, bool BWD>
__global__ __launch_bounds__(256) void maxpool2_kernel(const T* __restrict__ x, long long ldx, const T* __restrict__ dy,
                                                       long long lddy, T* __restrict__ out, long long ldo, int N, int D,
                                                       int H, int W, int C, int accumulate) {
    constexpr int WD = VEC ? DT<T>::EPC : 1;
    const int OD = D / 2, OH = H / 2, OW = W / 2;
    const int groups = (C + WD - 1) / WD;
    const unsigned total = (unsigned)((long long)N * OD * OH * OW * groups);   // < 2^31: checked by the host wrappers
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        // 32-bit index arithmetic: five 64-bit divisions per thread cost more than the eight loads
        const unsigned ug = (unsigned)groups;
        unsigned t = i / ug;
        const int g = (int)(i - t * ug);
        unsigned t2 = t / (unsigned)OW;
        const int ow = (int)(t - t2 * (unsigned)OW);
        t = t2 / (unsigned)OH;
        const int oh = (int)(t2 - t * (unsigned)OH);
        const int n = (int)(t / (unsigned)OD);
        const int od = (int)(t - (unsigned)n * (unsigned)OD);
        float best[WD];
        int arg[WD];
#pragma unroll
        for (int e = 0; e < WD; ++e) { best[e] = -INFINITY; arg[e] = 0; }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long vox = (((long long)n * D + 2 * od + (k >> 2)) * H + 2 * oh + ((k >> 1) & 1)) * W + 2 * ow + (k & 1);
            float v[WD];
            if constexpr (VEC) {
                ChunkV<T> c; c.load(x + vox * ldx + g * WD);
#pragma unroll
                for (int e = 0; e < WD; ++e) v[e] = c.v[e];
            } else {
                v[0] = DT<T>::ld(x + vox * ldx + g);
            }
#pragma unroll
            for (int e = 0; e < WD; ++e)
                if (v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; arg[e] = k; }
        }
        const long long ovox = (((long long)n * OD + od) * OH + oh) * OW + ow;
        if constexpr (!BWD) {
            if constexpr (VEC) {
                ChunkV<T> c;
#pragma unroll
                for (int e = 0; e < WD; ++e) c.v[e] = best[e];
                c.store(out + ovox * ldo + g * WD);
            } else {
                DT<T>::st(out + ovox * ldo + g, best[0]);
            }
        } else {
            float gv[WD];
            if constexpr (VEC) {
                ChunkV<T> c; c.load(dy + ovox * lddy + g * WD);
#pragma unroll
                for (int e = 0; e < WD; ++e) gv[e] = c.v[e];
            } else {
                gv[0] = DT<T>::ld(dy + ovox * lddy + g);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long long vox = (((long long)n * D + 2 * od + (k >> 2)) * H + 2 * oh + ((k >> 1) & 1)) * W + 2 * ow + (k & 1);
                T* dst = out + vox * ldo + g * WD;
                if constexpr (VEC) {
                    ChunkV<T> c;
                    if (accumulate) c.load(dst);
                    else {
#pragma unroll
                        for (int e = 0; e < WD; ++e) c.v[e] = 0.f;
                    }
#pragma unroll
                    for (int e = 0; e < WD; ++e) if (arg[e] == k) c.v[e] += gv[e];
                    c.store(dst);
                } else {
                    float base = accumulate ? DT<T>::ld(dst) : 0.f;
                    if (arg[0] == k) base += gv[0];
                    DT<T>::st(dst, base);
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int msseg_maxpool2_fwd(const void* x, long long ldx, void* y, long long ldy, int N, int D, int H, int W, int C,
                       int dtype, msseg_stream_t stream) {
    if (!x || !y || D < 2 || H < 2 || W < 2 || C < 1) MSSEG_FAIL(MSSEG_EINVAL, "maxpool2_fwd: bad args");
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    const bool vec = vec_ok(x, ldx, C, esz) && vec_ok(y, ldy, C, esz);
    const long long total = (long long)N * (D / 2) * (H / 2) * (W / 2) * ceil_div(C, vec ? 16 / esz : 1);
    if (total >= 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "maxpool2_fwd: too many elements");
    const int g = stream_grid(total);
#define MP_F(T_, V_) hipLaunchKernelGGL((maxpool2_kernel<T_, V_, false>), dim3(g), dim3(256), 0, (hipStream_t)stream, \
                                        (const T_*)x, ldx, (const T_*)nullptr, 0LL, (T_*)y, ldy, N, D, H, W, C, 0)
    const bool known = for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (vec) MP_F(T, true); else MP_F(T, false);
    });
    if (!known) return bad_dtype(dtype);
#undef MP_F
    MSSEG_CHECK_LAUNCH("maxpool2_fwd");
    return MSSEG_OK;
}

int msseg_maxpool2_bwd(const void* x, long long ldx, const void* dy, long long lddy, void* dx, long long lddx, int N,
                       int D, int H, int W, int C, int accumulate, int dtype, msseg_stream_t stream) {
    if (!x || !dy || !dx || D < 2 || H < 2 || W < 2 || C < 1) MSSEG_FAIL(MSSEG_EINVAL, "maxpool2_bwd: bad args");
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    const bool vec = vec_ok(x, ldx, C, esz) && vec_ok(dy, lddy, C, esz) && vec_ok(dx, lddx, C, esz);
    const long long total = (long long)N * (D / 2) * (H / 2) * (W / 2) * ceil_div(C, vec ? 16 / esz : 1);
    if (total >= 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "maxpool2_bwd: too many elements");
    const int g = stream_grid(total);
#define MP_B(T_, V_) hipLaunchKernelGGL((maxpool2_kernel<T_, V_, true>), dim3(g), dim3(256), 0, (hipStream_t)stream, \
                                        (const T_*)x, ldx, (const T_*)dy, lddy, (T_*)dx, lddx, N, D, H, W, C, accumulate)
    const bool known = for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (vec) MP_B(T, true); else MP_B(T, false);
    });
    if (!known) return bad_dtype(dtype);
#undef MP_B
    MSSEG_CHECK_LAUNCH("maxpool2_bwd");
    return MSSEG_OK;
}

}  // extern "C"
