// Swin 3-D shifted-window attention (forward + backward).
//
// Window attention replaces swin_nnformer.py:235-289 + :128-196 of the reference between the qkv Linear and the
// proj Linear:  pad -> roll(-shift) -> window_partition -> softmax(q k^T * scale + bias[+mask]) v -> window_reverse
// -> roll(+shift) -> crop.  Nothing is materialised: the kernel addresses tokens of the [B,S,H,W,3C] qkv tensor
// through the (shift, window, position) map, synthesises padded tokens (qkv = qkv bias), derives the -100 region
// mask from coordinates, and streams keys through LDS with an online softmax, so the [B_,h,N,N] score tensor
// never exists.  This is the exact-fp32-math version used for both dtypes (bf16 I/O, fp32 accumulate); one
// workgroup = one window, one thread = one query (forward / dQ) or one key (dK, dV).
#include "attention_common.h"

#include <stdlib.h>

using namespace msseg_attn;

namespace {

constexpr int HD_MAX = 32;

// ---------------------------------------------------------------------------------------------------------
// forward: grid (nW, B), block 256.  Loops heads; per head K,V of the window live in LDS (fp32).
// ---------------------------------------------------------------------------------------------------------
template <typename T, int HD>
__global__ __launch_bounds__(256) void win_attn_fwd_kernel(const AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* kS = (float*)smem;            // [N][HD]
    float* vS = kS + p.N * HD;           // [N][HD]
    float* tabS = vS + p.N * HD;         // [M3] bias table of the current head
    int* tok = (int*)(tabS + p.M3);      // [N] voxel index or -1
    int* regS = tok + p.N;               // [N]
    int* codeS = regS + p.N;             // [N]
    const int nW = p.nWs * p.nWh * p.nWw;
    const int m = 2 * p.bws - 1;
    const int off = ((p.bws - 1) * m + (p.bws - 1)) * m + (p.bws - 1);
    for (int wb = blockIdx.x; wb < p.nwin_total; wb += gridDim.x) {
        const int w = wb % nW, b = wb / nW;
        const int wx = w % p.nWw, wy = (w / p.nWw) % p.nWh, wz = w / (p.nWw * p.nWh);
        const T* qkv = (const T*)p.qkv + (long long)b * p.S * p.H * p.W * 3 * p.C;
        T* out = (T*)p.out + (long long)b * p.S * p.H * p.W * p.C;
        const float* table = p.table + b * p.tab_stride;
        __syncthreads();
        for (int i = threadIdx.x; i < p.N; i += 256) {
            int rg, cd;
            tok[i] = window_token(p, wz, wy, wx, i, rg, cd);
            regS[i] = rg;
            codeS[i] = cd;
        }
        for (int h = blockIdx.y; h < p.heads; h += gridDim.y) {
            __syncthreads();
            for (int i = threadIdx.x; i < p.M3; i += 256) tabS[i] = table[(long long)i * p.heads + h];
            for (int i = threadIdx.x; i < p.N * HD; i += 256) {
                const int j = i / HD, e = i % HD;
                const int t = tok[j];
                const int ck = p.C + h * HD + e, cv = 2 * p.C + h * HD + e;
                float kv, vv;
                if (t >= 0) {
                    kv = DT<T>::ld(qkv + (long long)t * 3 * p.C + ck);
                    vv = DT<T>::ld(qkv + (long long)t * 3 * p.C + cv);
                } else {
                    kv = p.qkv_bias ? p.qkv_bias[ck] : 0.f;
                    vv = p.qkv_bias ? p.qkv_bias[cv] : 0.f;
                    if (sizeof(T) == 2) { kv = (float)(bf16_t)kv; vv = (float)(bf16_t)vv; }
                }
                kS[i] = kv;
                vS[i] = vv;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < p.N; i += 256) {
                const int t = tok[i];
                float q[HD], o[HD];
#pragma unroll
                for (int e = 0; e < HD; ++e) {
                    float qv;
                    if (t >= 0) qv = DT<T>::ld(qkv + (long long)t * 3 * p.C + h * HD + e);
                    else {
                        qv = p.qkv_bias ? p.qkv_bias[h * HD + e] : 0.f;
                        if (sizeof(T) == 2) qv = (float)(bf16_t)qv;
                    }
                    q[e] = qv * p.scale;
                    o[e] = 0.f;
                }
                const int ri = regS[i], ci = codeS[i] + off;
                float mx = -INFINITY, l = 0.f;
                for (int j = 0; j < p.N; ++j) {
                    float sc = 0.f;
#pragma unroll
                    for (int e = 0; e < HD; ++e) sc += q[e] * kS[j * HD + e];
                    sc += tabS[ci - codeS[j]];
                    if (p.use_mask && regS[j] != ri) sc += -100.f;
                    const float mn = fmaxf(mx, sc);
                    const float a = expf(mx - mn), pe = expf(sc - mn);
                    l = l * a + pe;
#pragma unroll
                    for (int e = 0; e < HD; ++e) o[e] = o[e] * a + pe * vS[j * HD + e];
                    mx = mn;
                }
                const float inv = 1.f / l;
                p.lse[((long long)wb * p.heads + h) * p.N + i] = mx + logf(l);
                if (t >= 0) {
#pragma unroll
                    for (int e = 0; e < HD; ++e) DT<T>::st(out + (long long)t * p.C + h * HD + e, o[e] * inv);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// backward: grid (nW, B), block 256.  Per head: Q, K, V, dO rows, lse, delta in LDS; phase A thread = query
// (dQ, dbias), phase B thread = key (dK, dV).  Gradients of padded tokens are dropped (they are constants).
// ---------------------------------------------------------------------------------------------------------
template <typename T, int HD>
__global__ __launch_bounds__(256) void win_attn_bwd_kernel(const AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const bool two = p.bwd_two_phase;  // K and Q share one array, V and dO the other: K, V staged for phase A, Q, dO for phase B
    float* qS = (float*)smem;          // [N][HD]  (already scaled)
    float* kS = two ? qS : qS + p.N * HD;
    float* vS = kS + p.N * HD;
    float* dS = two ? vS : vS + p.N * HD;   // dO [N][HD]
    float* lseS = dS + p.N * HD;       // [N]
    float* delS = lseS + p.N;          // [N]  delta_i = dO_i . O_i
    float* tabS = delS + p.N;          // [M3]
    int* tok = (int*)(tabS + p.M3);
    int* regS = tok + p.N;
    int* codeS = regS + p.N;
    float* dtabS = (float*)(codeS + p.N);  // [M3] or [heads][M3]
    const int nW = p.nWs * p.nWh * p.nWw;
    const int m = 2 * p.bws - 1;
    const int off = ((p.bws - 1) * m + (p.bws - 1)) * m + (p.bws - 1);
    const long long vol = (long long)p.S * p.H * p.W;
    const int ndt = p.dtable ? (p.dtab_all_heads ? p.heads * p.M3 : p.M3) : 0;
    for (int i = threadIdx.x; i < ndt; i += 256) dtabS[i] = 0.f;
    for (int wb = blockIdx.x; wb < p.nwin_total; wb += gridDim.x) {
        const int w = wb % nW, b = wb / nW;
        const int wx = w % p.nWw, wy = (w / p.nWw) % p.nWh, wz = w / (p.nWw * p.nWh);
        const T* qkv = (const T*)p.qkv + b * vol * 3 * p.C;
        const T* outp = (const T*)p.out + b * vol * p.C;
        const T* dout = (const T*)p.dout + b * vol * p.C;
        T* dqkv = (T*)p.dqkv + b * vol * 3 * p.C;
        const float* table = p.table + b * p.tab_stride;
        __syncthreads();
        for (int i = threadIdx.x; i < p.N; i += 256) {
            int rg, cd;
            tok[i] = window_token(p, wz, wy, wx, i, rg, cd);
            regS[i] = rg;
            codeS[i] = cd;
        }
        for (int h = blockIdx.y; h < p.heads; h += gridDim.y) {
            __syncthreads();
            float* dtab = p.dtab_all_heads ? dtabS + h * p.M3 : dtabS;
            for (int i = threadIdx.x; i < p.M3; i += 256) tabS[i] = table[(long long)i * p.heads + h];
            // channel ch of [0, 3C) of token t (a padded token: the bias, rounded as a stored token would be); dO of a padded token is 0
            auto qkv_at = [&](int t, int ch) -> float {
                if (t >= 0) return DT<T>::ld(qkv + (long long)t * 3 * p.C + ch);
                float v = p.qkv_bias ? p.qkv_bias[ch] : 0.f;
                if (sizeof(T) == 2) v = (float)(bf16_t)v;
                return v;
            };
            auto dout_at = [&](int t, int c) -> float { return t >= 0 ? DT<T>::ld(dout + (long long)t * p.C + c) : 0.f; };
            for (int i = threadIdx.x; i < p.N * HD; i += 256) {
                const int j = i / HD, e = i % HD;
                const int t = tok[j];
                const int c = h * HD + e;
                if (!two) { qS[i] = qkv_at(t, c) * p.scale; dS[i] = dout_at(t, c); }
                kS[i] = qkv_at(t, p.C + c); vS[i] = qkv_at(t, 2 * p.C + c);
            }
            for (int i = threadIdx.x; i < p.N; i += 256) {
                lseS[i] = p.lse[((long long)wb * p.heads + h) * p.N + i];
                const int t = tok[i];
                float d = 0.f;
                if (t >= 0) {
#pragma unroll
                    for (int e = 0; e < HD; ++e)
                        d += DT<T>::ld(dout + (long long)t * p.C + h * HD + e) * DT<T>::ld(outp + (long long)t * p.C + h * HD + e);
                }
                delS[i] = d;
            }
            __syncthreads();
            // phase A: thread = query i -> dQ_i ; dtable[rel(i,j)] += dS_ij
            for (int i = threadIdx.x; i < p.N; i += 256) {
                float q[HD], dq[HD], dO[HD];
#pragma unroll
                for (int e = 0; e < HD; ++e) {
                    if (two) { q[e] = qkv_at(tok[i], h * HD + e) * p.scale; dO[e] = dout_at(tok[i], h * HD + e); }
                    else { q[e] = qS[i * HD + e]; dO[e] = dS[i * HD + e]; }
                    dq[e] = 0.f;
                }
                const float lse = lseS[i], del = delS[i];
                const int ri = regS[i], ci = codeS[i] + off;
                const bool live = tok[i] >= 0;
                for (int j = 0; j < p.N; ++j) {
                    float sc = 0.f, dp = 0.f;
#pragma unroll
                    for (int e = 0; e < HD; ++e) { sc += q[e] * kS[j * HD + e]; dp += dO[e] * vS[j * HD + e]; }
                    const int ti = ci - codeS[j];
                    sc += tabS[ti];
                    if (p.use_mask && regS[j] != ri) sc += -100.f;
                    const float pr = expf(sc - lse);
                    const float ds = pr * (dp - del);
#pragma unroll
                    for (int e = 0; e < HD; ++e) dq[e] += ds * kS[j * HD + e];
                    if (p.dtable && live) atomicAdd(&dtab[ti], ds);
                }
                const int t = tok[i];
                if (t >= 0) {
#pragma unroll
                    for (int e = 0; e < HD; ++e) DT<T>::st(dqkv + (long long)t * 3 * p.C + h * HD + e, dq[e] * p.scale);
                }
            }
            if (two) {   // every thread is done with K and V: Q and dO take their place
                __syncthreads();
                for (int i = threadIdx.x; i < p.N * HD; i += 256) {
                    const int t = tok[i / HD], c = h * HD + i % HD;
                    qS[i] = qkv_at(t, c) * p.scale; dS[i] = dout_at(t, c);
                }
                __syncthreads();
            }
            // phase B: thread = key j -> dK_j, dV_j
            for (int j = threadIdx.x; j < p.N; j += 256) {
                float k[HD], v[HD], dk[HD], dv[HD];
#pragma unroll
                for (int e = 0; e < HD; ++e) {
                    if (two) { k[e] = qkv_at(tok[j], p.C + h * HD + e); v[e] = qkv_at(tok[j], 2 * p.C + h * HD + e); }
                    else { k[e] = kS[j * HD + e]; v[e] = vS[j * HD + e]; }
                    dk[e] = dv[e] = 0.f;
                }
                const int rj = regS[j], cj = off - codeS[j];
                for (int i = 0; i < p.N; ++i) {
                    if (tok[i] < 0) continue;  // padded queries produce no output, hence no gradient
                    float sc = 0.f, dp = 0.f;
#pragma unroll
                    for (int e = 0; e < HD; ++e) { sc += qS[i * HD + e] * k[e]; dp += dS[i * HD + e] * v[e]; }
                    sc += tabS[codeS[i] + cj];
                    if (p.use_mask && regS[i] != rj) sc += -100.f;
                    const float pr = expf(sc - lseS[i]);
                    const float ds = pr * (dp - delS[i]);
#pragma unroll
                    for (int e = 0; e < HD; ++e) { dv[e] += pr * dS[i * HD + e]; dk[e] += ds * qS[i * HD + e]; }
                }
                const int t = tok[j];
                if (t >= 0) {
                    T* row = dqkv + (long long)t * 3 * p.C;
#pragma unroll
                    for (int e = 0; e < HD; ++e) {
                        DT<T>::st(row + p.C + h * HD + e, dk[e]);   // qS already carries the scale
                        DT<T>::st(row + 2 * p.C + h * HD + e, dv[e]);
                    }
                }
            }
            if (p.dtable && !p.dtab_all_heads) {
                __syncthreads();
                for (int i = threadIdx.x; i < p.M3; i += 256) {
                    const float v = dtabS[i];
                    if (v != 0.f) atomicAdd(&p.dtable[b * p.tab_stride + (long long)i * p.heads + h], v);
                    dtabS[i] = 0.f;
                }
            }
        }
    }
    if (p.dtable && p.dtab_all_heads) {   // (never with per-sample tables: the host clears dtab_all_heads for them)
        __syncthreads();
        for (int i = threadIdx.x; i < p.heads * p.M3; i += 256) {
            const float v = dtabS[i];
            const int h = i / p.M3, e = i % p.M3;
            if (v != 0.f) atomicAdd(&p.dtable[(long long)e * p.heads + h], v);
        }
    }
}

int fill_attn(AttnParams& p, int B, int S, int H, int W, int C, int heads, int ws, int shift, int bias_ws) {
    if (B < 1 || S < 1 || H < 1 || W < 1 || heads < 1 || C % heads || ws < 1 || shift < 0 || shift >= ws)
        MSSEG_FAIL(MSSEG_EINVAL, "window_attention: bad shape");
    if (bias_ws == 0) bias_ws = ws;
    if (bias_ws < ws) MSSEG_FAIL(MSSEG_EINVAL, "window_attention: bias window %d smaller than the window %d", bias_ws, ws);
    p.bws = bias_ws;
    p.B = B; p.S = S; p.H = H; p.W = W; p.C = C; p.heads = heads; p.hd = C / heads; p.ws = ws; p.shift = shift;
    p.nWs = ceil_div(S, ws); p.nWh = ceil_div(H, ws); p.nWw = ceil_div(W, ws);
    p.Sp = p.nWs * ws; p.Hp = p.nWh * ws; p.Wp = p.nWw * ws;
    p.N = ws * ws * ws;
    p.M3 = (2 * bias_ws - 1) * (2 * bias_ws - 1) * (2 * bias_ws - 1);
    p.nwin_total = p.nWs * p.nWh * p.nWw * B;
    p.scale = 1.0f / sqrtf((float)p.hd);
    p.use_mask = shift > 0;
    if (p.hd != 8 && p.hd != 16 && p.hd != 32) MSSEG_FAIL(MSSEG_EINVAL, "window_attention: head_dim %d not in {8,16,32}", p.hd);
    if (p.N > 512) MSSEG_FAIL(MSSEG_EINVAL, "window_attention: window of %d tokens too large", p.N);
    return MSSEG_OK;
}

// KERN<dtype's T, head dim>; returns from the entry point on a failed LDS setting or a dtype that is neither code
#define ATTN_LAUNCH(KERN, SMEM, WHO)                                                                     \
    do {                                                                                                 \
        int rc__ = MSSEG_OK;                                                                             \
        const bool known__ = for_dtype(dtype, [&](auto t__) {                                            \
            using T_ = typename decltype(t__)::type;                                                     \
            int gx__ = p.nwin_total < msseg_num_cus() * 2 ? p.nwin_total : msseg_num_cus() * 2;          \
            int gy__ = (msseg_num_cus() * 2 + gx__ - 1) / gx__;                                          \
            if (gy__ > p.heads) gy__ = p.heads;                                                          \
            if (p.dtab_all_heads) gy__ = 1;                                                              \
            dim3 grid(gx__, gy__);                                                                       \
            if (p.hd == 8) { if (!(rc__ = attn_set_lds((const void*)KERN<T_, 8>, SMEM)))                 \
                hipLaunchKernelGGL((KERN<T_, 8>), grid, dim3(256), SMEM, (hipStream_t)stream, p); }      \
            else if (p.hd == 16) { if (!(rc__ = attn_set_lds((const void*)KERN<T_, 16>, SMEM)))          \
                hipLaunchKernelGGL((KERN<T_, 16>), grid, dim3(256), SMEM, (hipStream_t)stream, p); }     \
            else { if (!(rc__ = attn_set_lds((const void*)KERN<T_, 32>, SMEM)))                          \
                hipLaunchKernelGGL((KERN<T_, 32>), grid, dim3(256), SMEM, (hipStream_t)stream, p); }     \
        });                                                                                              \
        if (!known__) MSSEG_FAIL(MSSEG_EINVAL, WHO ": bad dtype");                                       \
        if (rc__) return rc__;                                                                           \
    } while (0)

}  // namespace

extern "C" {

static int attn_set_lds(const void* kern, size_t smem) {
    if (smem > 64 * 1024 &&
        hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        MSSEG_FAIL(MSSEG_ELAUNCH, "window_attention: cannot set %zu bytes of dynamic LDS", smem);
    return MSSEG_OK;
}

static int check_tab_stride(const AttnParams& p, long long table_stride) {
    if (table_stride != 0 && table_stride < (long long)p.M3 * p.heads)
        MSSEG_FAIL(MSSEG_EINVAL, "window_attention: table stride %lld smaller than one table (%d x %d)", table_stride, p.M3,
                   p.heads);
    return MSSEG_OK;
}

int msseg_window_attention_fwd(const void* qkv, const float* qkv_bias, const float* table, void* out, float* lse, int B,
                               int S, int H, int W, int C, int heads, int ws, int shift, int bias_ws, long long table_stride,
                               int dtype, msseg_stream_t stream) {
    if (!qkv || !table || !out || !lse) MSSEG_FAIL(MSSEG_EINVAL, "window_attention_fwd: null pointer");
    AttnParams p{};
    if (int rc = fill_attn(p, B, S, H, W, C, heads, ws, shift, bias_ws)) return rc;
    if (int rc = check_tab_stride(p, table_stride)) return rc;
    p.qkv = qkv; p.qkv_bias = qkv_bias; p.table = table; p.out = out; p.lse = lse; p.tab_stride = table_stride;
    const size_t smem = (size_t)p.N * p.hd * 2 * 4 + (size_t)p.M3 * 4 + (size_t)p.N * 3 * 4;
    if (smem > 160 * 1024) MSSEG_FAIL(MSSEG_EINVAL, "window_attention_fwd: window too large for LDS");
    if (dtype == MSSEG_BF16 && (p.hd == 16 || p.hd == 32) && p.N <= 352 && p.M3 <= 4095 && (C % 8) == 0 &&
        !getenv("MSSEG_ATTN_NO_MFMA")) {
        // bf16: QK^T and PV on the matrix cores (attention_mfma.hip)
        return msseg_window_attention_fwd_mfma(p, (hipStream_t)stream);
    }
    ATTN_LAUNCH(win_attn_fwd_kernel, smem, "window_attention_fwd");
    MSSEG_CHECK_LAUNCH("window_attention_fwd");
    return MSSEG_OK;
}

static bool attn_bwd_on_mfma(const AttnParams& p, int C, int dtype) {
    {   // LDS image of the MFMA backward (attention_mfma.hip launch_bwd): head dim 32 at 343 tokens does not fit
        const int nkt = (p.N + 31) / 32;
        const size_t np = (size_t)(nkt == 1 ? 1 : (nkt == 2 ? 2 : (nkt <= 4 ? 4 : (nkt <= 7 ? 7 : 11)))) * 32;
        if (7 * np * p.hd * 2 + 2 * np * 4 + (size_t)2 * p.M3 * 4 + np * 8 + 16 > 160 * 1024) return false;
    }
    return dtype == MSSEG_BF16 && (p.hd == 16 || p.hd == 32) && p.N <= 352 && p.M3 <= 4095 && (C % 8) == 0 &&
           !getenv("MSSEG_ATTN_NO_MFMA");
}

size_t msseg_window_attention_bwd_workspace_bytes(int B, int S, int H, int W, int C, int heads, int ws, int shift,
                                                  int bias_ws, long long table_stride, int dtype) {
    AttnParams p{};
    if (fill_attn(p, B, S, H, W, C, heads, ws, shift, bias_ws) != MSSEG_OK) return 0;
    p.tab_stride = table_stride;
    if (!attn_bwd_on_mfma(p, C, dtype) || getenv("MSSEG_ATTN_BWD_NO_WS")) return 0;
    return msseg_window_attention_bwd_mfma_ws_bytes(p);
}

int msseg_window_attention_bwd(const void* qkv, const float* qkv_bias, const float* table, const void* out,
                               const float* lse, const void* dout, void* dqkv, float* dtable, int B, int S, int H, int W,
                               int C, int heads, int ws, int shift, int bias_ws, long long table_stride, int dtype,
                               void* workspace, size_t workspace_bytes, msseg_stream_t stream) {
    if (!qkv || !table || !out || !lse || !dout || !dqkv) MSSEG_FAIL(MSSEG_EINVAL, "window_attention_bwd: null pointer");
    AttnParams p{};
    if (int rc = fill_attn(p, B, S, H, W, C, heads, ws, shift, bias_ws)) return rc;
    if (int rc = check_tab_stride(p, table_stride)) return rc;
    p.qkv = qkv; p.qkv_bias = qkv_bias; p.table = table; p.out = (void*)out; p.lse = (float*)lse; p.dout = dout;
    p.dqkv = dqkv; p.dtable = dtable; p.tab_stride = table_stride;
    if (attn_bwd_on_mfma(p, C, dtype)) {
        // bf16: all five contractions of the backward on the matrix cores (attention_mfma.hip); with a workspace the
        // table gradient is a window sum + gather instead of LDS float atomics
        if (workspace != nullptr && dtable != nullptr) {
            if (workspace_bytes < msseg_window_attention_bwd_mfma_ws_bytes(p))
                MSSEG_FAIL(MSSEG_EINVAL, "window_attention_bwd: workspace too small (%zu < %zu bytes)", workspace_bytes,
                           msseg_window_attention_bwd_mfma_ws_bytes(p));
            msseg_window_attention_bwd_mfma_carve(p, workspace);
        }
        return msseg_window_attention_bwd_mfma(p, (hipStream_t)stream);
    }
    size_t base = (size_t)p.N * p.hd * 4 * 4 + (size_t)p.N * 5 * 4 + (size_t)p.M3 * 4;
    // Q, K, V, dO of one head do not fit together (head dim 32 at 343 tokens): two arrays, staged once per phase
    p.bwd_two_phase = base + (size_t)p.M3 * 4 > 160 * 1024 ? 1 : 0;
    if (p.bwd_two_phase) base -= (size_t)p.N * p.hd * 2 * 4;
    // (per-sample tables: the LDS sums are flushed after every (window, head), into the table of that window's sample)
    p.dtab_all_heads = (table_stride == 0 && base + (size_t)heads * p.M3 * 4 <= 96 * 1024) ? 1 : 0;
    const size_t smem = base + (size_t)(p.dtab_all_heads ? heads : 1) * p.M3 * 4;
    if (smem > 160 * 1024) MSSEG_FAIL(MSSEG_EINVAL, "window_attention_bwd: window too large for LDS (%zu bytes)", smem);
    ATTN_LAUNCH(win_attn_bwd_kernel, smem, "window_attention_bwd");
    MSSEG_CHECK_LAUNCH("window_attention_bwd");
    return MSSEG_OK;
}

}  // extern "C"
