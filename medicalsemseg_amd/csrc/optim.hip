// The optimiser step: AdamW over a flat fp32 parameter buffer, and the gradient norm of clip_grad_norm_ in a fixed order.
#include "common.h"

namespace {

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, const uint8_t* __restrict__ decay, long long n, float lr, float b1,
                             float b2, float eps, float wd, float bc1, float bc2_sqrt, const float* gscale,
                             const float* hyper) {
    const float gs = gscale ? gscale[0] : 1.f;
    if (hyper) {  // device-resident (lr, step): lets a captured hipGraph replay with a changing schedule
        lr = hyper[0];
        const float st = hyper[1];
        bc1 = 1.f - powf(b1, st);
        bc2_sqrt = sqrtf(1.f - powf(b2, st));
    }
    // four parameters per thread (16-byte accesses) when the buffers allow it; scalar tail / unaligned fallback
    const bool vec = (n % 4 == 0) && ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) &&
                     (!decay || (((uintptr_t)decay & 3) == 0));
    const long long nv = vec ? n / 4 : 0;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        f32x4_t pi = ((const f32x4_t*)p)[i], mi = ((const f32x4_t*)m)[i], vi = ((const f32x4_t*)v)[i];
        const f32x4_t gi = ((const f32x4_t*)g)[i];
        const uint32_t dm = decay ? ((const uint32_t*)decay)[i] : 0x01010101u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ge = gi[e] * gs;
            float pe = pi[e];
            if ((dm >> (8 * e)) & 0xffu) pe *= (1.f - lr * wd);
            const float me = b1 * mi[e] + (1.f - b1) * ge;
            const float ve = b2 * vi[e] + (1.f - b2) * ge * ge;
            mi[e] = me; vi[e] = ve;
            const float denom = sqrtf(ve) / bc2_sqrt + eps;
            pi[e] = pe - (lr / bc1) * (me / denom);
        }
        ((f32x4_t*)m)[i] = mi; ((f32x4_t*)v)[i] = vi; ((f32x4_t*)p)[i] = pi;
    }
    for (long long i = nv * 4 + blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float gi = g[i] * gs;
        float pi = p[i];
        if (!decay || decay[i]) pi *= (1.f - lr * wd);
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pi - (lr / bc1) * (mi / denom);
    }
}

// Sum of squares (the gradient norm of clip_grad_norm_) in a fixed order: per-block partials, then one block adds them.  The float
// atomicAdd this replaces made the clipping scale -- and with it every parameter of a clipped step -- differ in the last bit from
// run to run.  The partial rows live in a buffer of the caller (nothing here is shared between calls).
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, long long n, float* __restrict__ part) {
    __shared__ float red[4];
    float s = 0.f;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += x[i] * x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void sumsq_finalize_kernel(const float* __restrict__ part, int nblk, float* out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

}  // namespace

extern "C" {

int msseg_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                     long long n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                     const float* grad_scale, const float* dev_hyper, msseg_stream_t stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n < 1 || (step < 1 && !dev_hyper))
        MSSEG_FAIL(MSSEG_EINVAL, "adamw_step: bad args");
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2 = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_kernel, dim3(stream_grid(n, 1024)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, decay_mask, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale, dev_hyper);
    MSSEG_CHECK_LAUNCH("adamw_step");
    return MSSEG_OK;
}

int msseg_sumsq(const float* x, long long n, float* out, float* partials, int n_partials, msseg_stream_t stream) {
    if (!x || !out || !partials || n < 1 || n_partials < 1) MSSEG_FAIL(MSSEG_EINVAL, "sumsq: bad args");
    int nblk = stream_grid(n, 4096);
    if (nblk > n_partials) nblk = n_partials;
    hipLaunchKernelGGL(sumsq_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, n, partials);
    MSSEG_CHECK_LAUNCH("sumsq");
    hipLaunchKernelGGL(sumsq_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partials, nblk, out);
    MSSEG_CHECK_LAUNCH("sumsq_finalize");
    return MSSEG_OK;
}

}  // extern "C"
