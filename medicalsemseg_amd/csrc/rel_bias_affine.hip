// Spacing-conditioned relative position bias (the reference's `rel_pos_bias_affine`, swin_nnformer.py:89-97, :157-166).
//
// The reference adds lin(emb[rel(i, j), h, :] * a[b, :]) to every logit of every window of sample b, with a learned
// emb [M3][heads][3], lin = nn.Linear(3, 1) and a [B][3] the voxel spacing (diagonal of the affine).  The term depends on
// (b, r = rel(i, j), h) only, so it folds into one bias table per sample:
//
//     T[b][r][h] = table[r][h] + lin.b + sum_k c[b][k] * emb[r][h][k],   c[b][k] = lin.w[k] * a[b][k]
//
// and the window-attention kernels read table b of window b * nW + w (AttnParams::tab_stride).  Their backward leaves the
// per-sample table gradient dT[b][r][h]; the parameter gradients follow from it:
//
//     dtable = sum_b dT_b,   demb[r][h][k] = sum_b c[b][k] dT_b[r][h],
//     dlin.w[k] = sum_b a[b][k] sum_{r,h} emb[r][h][k] dT_b[r][h],   dlin.b = sum_{b,r,h} dT_b[r][h]
//
// Every sum runs in a fixed order (no float atomics): the results are bit-identical from run to run.  The gradient is two
// launches: one thread per table entry (dtable, demb and per-workgroup partial sums of dlin), then one workgroup that adds
// the partial rows in workgroup order (dlin.w, dlin.b).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void rel_bias_affine_fold_kernel(const float* __restrict__ table,
                                                                   const float* __restrict__ emb,
                                                                   const float* __restrict__ lin_w,
                                                                   const float* __restrict__ lin_b,
                                                                   const float* __restrict__ aff, float* __restrict__ T,
                                                                   int B, int n) {
    const float w0 = lin_w[0], w1 = lin_w[1], w2 = lin_w[2], lb = lin_b[0];
    const long long total = (long long)B * n;
    for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int b = (int)(idx / n), i = (int)(idx % n);
        const float c0 = w0 * aff[b * 3 + 0], c1 = w1 * aff[b * 3 + 1], c2 = w2 * aff[b * 3 + 2];
        float v = table[i] + lb;
        v += c0 * emb[3LL * i + 0];
        v += c1 * emb[3LL * i + 1];
        v += c2 * emb[3LL * i + 2];
        T[idx] = v;
    }
}

// thread = table entry (r, h): its dtable / demb outputs, and its share of the four scalar sums (dlin.w, dlin.b), reduced
// over the workgroup by a fixed tree into one partial row per workgroup
__global__ __launch_bounds__(256) void rel_bias_affine_grad_kernel(const float* __restrict__ dT, const float* __restrict__ emb,
                                                                   const float* __restrict__ lin_w,
                                                                   const float* __restrict__ aff, float* __restrict__ dtable,
                                                                   float* __restrict__ demb, float* __restrict__ part, int B,
                                                                   int n, int flags) {
    __shared__ float red[4][256];
    const int tid = threadIdx.x;
    const float w0 = lin_w[0], w1 = lin_w[1], w2 = lin_w[2];
    float u0 = 0.f, u1 = 0.f, u2 = 0.f, ub = 0.f;
    for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
        float t = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
        for (int b = 0; b < B; ++b) {
            const float d = dT[(long long)b * n + i];
            const float a0 = aff[b * 3 + 0], a1 = aff[b * 3 + 1], a2 = aff[b * 3 + 2];
            t += d;
            e0 += (w0 * a0) * d; e1 += (w1 * a1) * d; e2 += (w2 * a2) * d;
            g0 += a0 * d; g1 += a1 * d; g2 += a2 * d;
        }
        if (dtable) dtable[i] = (flags & MSSEG_AFFINE_ACC_TABLE) ? dtable[i] + t : t;
        if (demb) {
            float* de = demb + 3LL * i;
            if (flags & MSSEG_AFFINE_ACC_EMB) { de[0] += e0; de[1] += e1; de[2] += e2; }
            else { de[0] = e0; de[1] = e1; de[2] = e2; }
        }
        u0 += emb[3LL * i + 0] * g0;
        u1 += emb[3LL * i + 1] * g1;
        u2 += emb[3LL * i + 2] * g2;
        ub += t;
    }
    red[0][tid] = u0; red[1][tid] = u1; red[2][tid] = u2; red[3][tid] = ub;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + s];
        }
        __syncthreads();
    }
    if (tid < 4) part[blockIdx.x * 4 + tid] = red[tid][0];
}

// one workgroup: the partial rows of the workgroups above, in workgroup order, then a fixed tree
__global__ __launch_bounds__(256) void rel_bias_affine_grad_finish_kernel(const float* __restrict__ part, int nblk,
                                                                          float* __restrict__ dlin_w,
                                                                          float* __restrict__ dlin_b, int flags) {
    __shared__ float red[4][256];
    const int tid = threadIdx.x;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = tid; k < nblk; k += 256) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += part[k * 4 + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + s];
        }
        __syncthreads();
    }
    if (tid < 3 && dlin_w) dlin_w[tid] = (flags & MSSEG_AFFINE_ACC_LIN_W) ? dlin_w[tid] + red[tid][0] : red[tid][0];
    if (tid == 3 && dlin_b) dlin_b[0] = (flags & MSSEG_AFFINE_ACC_LIN_B) ? dlin_b[0] + red[3][0] : red[3][0];
}

constexpr int GRAD_MAX_BLOCKS = 1024;

int grad_blocks(int n) {
    const int b = (n + 255) / 256;
    return b < GRAD_MAX_BLOCKS ? b : GRAD_MAX_BLOCKS;
}

}  // namespace

extern "C" {

int msseg_rel_bias_affine_fold(const float* table, const float* emb, const float* lin_w, const float* lin_b,
                               const float* aff, float* T, int B, int M3, int heads, msseg_stream_t stream) {
    if (!table || !emb || !lin_w || !lin_b || !aff || !T) MSSEG_FAIL(MSSEG_EINVAL, "rel_bias_affine_fold: null pointer");
    if (B < 1 || M3 < 1 || heads < 1) MSSEG_FAIL(MSSEG_EINVAL, "rel_bias_affine_fold: bad shape");
    const int n = M3 * heads;
    long long blocks = ((long long)B * n + 255) / 256;
    const long long cap = (long long)msseg_num_cus() * 4;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(rel_bias_affine_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table, emb,
                       lin_w, lin_b, aff, T, B, n);
    MSSEG_CHECK_LAUNCH("rel_bias_affine_fold");
    return MSSEG_OK;
}

size_t msseg_rel_bias_affine_grad_workspace_bytes(int M3, int heads) {
    if (M3 < 1 || heads < 1) return 0;
    return (size_t)grad_blocks(M3 * heads) * 4 * sizeof(float);
}

int msseg_rel_bias_affine_grad(const float* dT, const float* emb, const float* lin_w, const float* aff, float* dtable,
                               float* demb, float* dlin_w, float* dlin_b, int B, int M3, int heads, int flags,
                               void* workspace, size_t workspace_bytes, msseg_stream_t stream) {
    if (!dT || !emb || !lin_w || !aff || !workspace) MSSEG_FAIL(MSSEG_EINVAL, "rel_bias_affine_grad: null pointer");
    if (B < 1 || M3 < 1 || heads < 1) MSSEG_FAIL(MSSEG_EINVAL, "rel_bias_affine_grad: bad shape");
    if (workspace_bytes < msseg_rel_bias_affine_grad_workspace_bytes(M3, heads))
        MSSEG_FAIL(MSSEG_EWORKSPACE, "rel_bias_affine_grad: workspace too small (%zu < %zu bytes)", workspace_bytes,
                   msseg_rel_bias_affine_grad_workspace_bytes(M3, heads));
    const int n = M3 * heads, nblk = grad_blocks(n);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(rel_bias_affine_grad_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, dT, emb, lin_w, aff, dtable,
                       demb, part, B, n, flags);
    MSSEG_CHECK_LAUNCH("rel_bias_affine_grad");
    hipLaunchKernelGGL(rel_bias_affine_grad_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)part, nblk,
                       dlin_w, dlin_b, flags);
    MSSEG_CHECK_LAUNCH("rel_bias_affine_grad_finish");
    return MSSEG_OK;
}

}  // extern "C"
