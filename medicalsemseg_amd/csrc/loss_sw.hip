// Segmentation losses -- Dice + cross-entropy, Tversky, Dice + focal -- as one pass over logits/labels forward and one
// pass backward (the loss kind is a compile-time parameter of the same kernels, and so is REGIONS: one sigmoid output per
// overlapping label region instead of a softmax over exclusive classes), hard Dice metric counts, and the sliding-window
// gather / blend / normalise kernels.
#include <type_traits>

#include "common.h"

namespace {

enum { LAB_F32 = 0, LAB_BF16 = 1, LAB_U8 = 2, LAB_I64 = 3 };
// what slots 1 and 3 of partial[n][c][0..3] hold: (sum p^2, -sum t*log p) | (sum p, unused) | (sum p^2, sum focal)
enum { KIND_DICE_CE = MSSEG_LOSS_DICE_CE, KIND_TVERSKY = MSSEG_LOSS_TVERSKY, KIND_DICE_FOCAL = MSSEG_LOSS_DICE_FOCAL };

MSSEG_DEVFN int load_label(const void* labels, int label_dtype, long long idx) {
    switch (label_dtype) {
        case LAB_F32: return (int)((const float*)labels)[idx];
        case LAB_BF16: return (int)(float)((const bf16_t*)labels)[idx];
        case LAB_U8: return (int)((const uint8_t*)labels)[idx];
        default: return (int)((const long long*)labels)[idx];
    }
}

// a 16-byte logits row (channels-last, ld * sizeof(T) == 16, what the networks' logits buffers are): ONE vector load per
// voxel instead of one 2-byte load per class
template <typename T, int CMAX>
MSSEG_DEVFN void unpack_row(const u32x4_t raw, int C, float* x) {
    constexpr int EPC = DT<T>::EPC;
    float v[EPC];
    if constexpr (sizeof(T) == 2) {
        const bf16x8_t h = __builtin_bit_cast(bf16x8_t, raw);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = (float)h[e];
    } else {
        const f32x4_t f = __builtin_bit_cast(f32x4_t, raw);
#pragma unroll
        for (int e = 0; e < EPC; ++e) v[e] = f[e];
    }
#pragma unroll
    for (int c = 0; c < CMAX; ++c) x[c] = (c < C && c < EPC) ? v[c < EPC ? c : 0] : -INFINITY;
}

template <typename T, int CMAX>
MSSEG_DEVFN void load_logits(const T* base, long long ld, long long S, int C, long long n, long long s, float* x) {
    // ld > 0: channels-last [N][S][ld]; ld == 0: NCDHW [N][C][S]
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c < C) x[c] = ld > 0 ? DT<T>::ld(base + (n * S + s) * ld + c) : DT<T>::ld(base + (n * C + c) * S + s);
        else x[c] = -INFINITY;
    }
}

template <int CMAX> MSSEG_DEVFN void softmax_inplace(float* x, int C, float& lse) {
    float mx = x[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c) mx = fmaxf(mx, x[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        x[c] = (c < C) ? expf(x[c] - mx) : 0.f;
        sum += x[c];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) x[c] *= inv;
    lse = mx + logf(sum);
}

// Sigmoid focal loss (gamma = 2) of ONE logit x against its one-hot target t, as MONAI's FocalLoss computes it inside
// DiceFocalLoss (which does not hand its softmax flag on): bce = x - x*t - logsigmoid(x), weight = exp(2 * logsigmoid(z))
// with z = -x * (2t - 1).  L = log1p(exp(-|x|)) serves both: logsigmoid(v) = min(v, 0) - L for v = +-x.
MSSEG_DEVFN float focal_value(float x, float t) {
    const float L = log1pf(expf(-fabsf(x)));
    const float bce = fmaxf(x, 0.f) - x * t + L;
    const float z = t > 0.f ? -x : x;
    return expf(2.f * (fminf(z, 0.f) - L)) * bce;
}

// d focal_value / d x.  With s = sigmoid(z), b = softplus(z) = bce: f = s^2 * b, df/dz = s^2 * (2 * (1 - s) * b + s),
// dz/dx = -1 where t = 1 and +1 elsewhere; 1 - s = sigmoid(-z) comes from its own logsigmoid, not from a subtraction.
MSSEG_DEVFN float focal_grad(float x, float t) {
    const float L = log1pf(expf(-fabsf(x)));
    const float z = t > 0.f ? -x : x;
    const float b = fmaxf(z, 0.f) + L;
    const float s = expf(fminf(z, 0.f) - L), s1 = expf(fminf(-z, 0.f) - L);
    const float dz = s * s * (2.f * s1 * b + s);
    return t > 0.f ? -dz : dz;
}

// REGIONS: target of channel c at a voxel with label value lab -- is lab in region c?  The masks are kernel arguments (scalar
// registers), c is a compile-time index in every caller: no table load.  A label outside 0..31 is in no region.
MSSEG_DEVFN float region_target(const msseg_region_masks& rm, int c, int lab) {
    return ((unsigned)lab < 32u && ((rm.mask[c] >> (lab & 31)) & 1u)) ? 1.f : 0.f;
}

// p = sigmoid(x), q = sigmoid(-x) = 1 - p (each from its own quotient, not from a subtraction) and L = log1p(exp(-|x|)), the
// softplus tail that BCEWithLogits = max(x, 0) - x*t + L needs
MSSEG_DEVFN void sigmoid_parts(float x, float& p, float& q, float& L) {
    const float e = expf(-fabsf(x));
    const float r = 1.f / (1.f + e), er = e * r;
    L = log1pf(e);
    p = x >= 0.f ? r : er;
    q = x >= 0.f ? er : r;
}

// partial[n][c][0..3] += (sum p*t, sum p^2, sum t, -sum t*log p); hard[n][c][0..2] += (|P&T|, |P|, |T|)
// (KIND_TVERSKY: slot 1 is sum p, slot 3 stays 0; KIND_DICE_FOCAL: slot 3 is the sum of the focal values)
// REGIONS: p = sigmoid(x[c]) and t = region_target per channel, slot 3 of KIND_DICE_CE is the sum of the BCE values, the
// hard prediction of channel c is x[c] > 0
template <typename T, int CMAX, int KIND, bool REGIONS>
__global__ __launch_bounds__(256) void dice_ce_partials_kernel(const T* __restrict__ logits, long long ld,
                                                               const void* __restrict__ labels, int label_dtype,
                                                               float* partial, float* hard, long long S, int C,
                                                               long long vox_per_block, float* rows,
                                                               const msseg_region_masks rm) {
    __shared__ float red[4][CMAX * 7];
    const long long n = blockIdx.y;
    const long long s0 = (long long)blockIdx.x * vox_per_block;
    long long s1 = s0 + vox_per_block;
    if (s1 > S) s1 = S;
    float acc[CMAX][7];
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[c][k] = 0.f;
    // four voxels per trip, their rows and labels requested before the first is used (a loop of one voxel per trip kept a
    // single 2-byte load in flight per class: 1.3 TB/s); the per-thread order of the voxels, and with it every sum, is unchanged
    const bool vec = ld > 0 && ld * (long long)sizeof(T) == 16 && C <= DT<T>::EPC && (((uintptr_t)logits) & 15) == 0;
    auto one = [&](float* x, int lab) {
        if constexpr (REGIONS) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if (c < C) {
                    const float t = region_target(rm, c, lab);
                    float p, q, L;
                    sigmoid_parts(x[c], p, q, L);
                    acc[c][0] += p * t;
                    if constexpr (KIND == KIND_TVERSKY) acc[c][1] += p;
                    else acc[c][1] += p * p;
                    acc[c][2] += t;
                    if constexpr (KIND == KIND_DICE_CE) acc[c][3] += fmaxf(x[c], 0.f) - x[c] * t + L;
                    else if constexpr (KIND == KIND_DICE_FOCAL) acc[c][3] += focal_value(x[c], t);
                    const float pm = x[c] > 0.f ? 1.f : 0.f;
                    acc[c][4] += pm * t;
                    acc[c][5] += pm;
                    acc[c][6] += t;
                }
            }
            return;
        }
        int am = 0;
        float best = x[0];
#pragma unroll
        for (int c = 1; c < CMAX; ++c)
            if (c < C && x[c] > best) { best = x[c]; am = c; }
        float raw[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) raw[c] = x[c];
        float lse;
        softmax_inplace<CMAX>(x, C, lse);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c < C) {
                const float t = (lab == c) ? 1.f : 0.f;
                acc[c][0] += x[c] * t;
                if constexpr (KIND == KIND_TVERSKY) acc[c][1] += x[c];
                else acc[c][1] += x[c] * x[c];
                acc[c][2] += t;
                if constexpr (KIND == KIND_DICE_CE) acc[c][3] += t * (lse - raw[c]);
                else if constexpr (KIND == KIND_DICE_FOCAL) acc[c][3] += focal_value(raw[c], t);
                const float pm = (am == c) ? 1.f : 0.f;
                acc[c][4] += pm * t;
                acc[c][5] += pm;
                acc[c][6] += t;
            }
        }
    };
    for (long long s = s0 + threadIdx.x; s < s1; s += 1024) {
        if (vec) {
            u32x4_t rows4[4];
            int lab4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long sj = s + 256 * j;
                rows4[j] = u32x4_t{0u, 0u, 0u, 0u};
                lab4[j] = 0;
                if (sj < s1) {
                    rows4[j] = *(const u32x4_t*)(logits + (n * S + sj) * ld);
                    lab4[j] = load_label(labels, label_dtype, n * S + sj);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (s + 256 * j < s1) {
                    float x[CMAX];
                    unpack_row<T, CMAX>(rows4[j], C, x);
                    one(x, lab4[j]);
                }
            }
        } else {
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const long long sj = s + 256 * j;
                if (sj < s1) {
                    float x[CMAX];
                    load_logits<T, CMAX>(logits, ld, S, C, n, sj, x);
                    one(x, load_label(labels, label_dtype, n * S + sj));
                }
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const float v = wave_sum(acc[c][k]);
            if (lane == 0) red[wave][c * 7 + k] = v;
        }
    __syncthreads();
    for (int i = threadIdx.x; i < C * 7; i += 256) {
        const float v = red[0][i] + red[1][i] + red[2][i] + red[3][i];
        const int c = i / 7, k = i % 7;
        if (rows) {   // deterministic mode: one row per block, summed in a fixed order by dice_ce_rows_finalize_kernel
            rows[((long long)n * gridDim.x + blockIdx.x) * (C * 7) + i] = v;
            continue;
        }
        if (k < 4) {
            if (partial) atomicAdd(&partial[(n * C + c) * 4 + k], v);
        } else if (hard) {
            atomicAdd(&hard[(n * C + c) * 3 + (k - 4)], v);
        }
    }
}

// loss[0..2] = (total, first term, second term) from the N*C rows of sums at `sums` (`stride` floats apart):
// (dice + ce, dice, ce) | (tversky, tversky, 0) | (dice + focal, dice, focal); one thread, fixed order.  regions: the sums are
// those of the sigmoid kinds (the same expressions; only the count behind the mean of slot 3 differs)
template <int KIND>
MSSEG_DEVFN void loss_triple(const float* sums, int stride, float* loss, int N, long long S, int C, float snr, float sdr,
                             float alpha, float beta, int regions) {
    float dice = 0.f, ce = 0.f;
    for (int i = 0; i < N * C; ++i) {
        const float I = sums[i * stride + 0], p2 = sums[i * stride + 1], t = sums[i * stride + 2];
        if constexpr (KIND == KIND_TVERSKY) {   // p2 is sum p here
            const float fp = alpha * (p2 - I), fn = beta * (t - I);
            dice += 1.f - (I + snr) / (I + fp + fn + sdr);
        } else {
            dice += 1.f - (2.f * I + snr) / (p2 + t + sdr);
            ce += sums[i * stride + 3];
        }
    }
    dice /= (float)(N * C);
    // the softmax cross-entropy has one term per voxel, the regions' BCE one per voxel and channel
    if constexpr (KIND == KIND_DICE_CE) ce /= (float)(regions ? (double)N * (double)C * (double)S : (double)N * (double)S);
    else if constexpr (KIND == KIND_DICE_FOCAL) ce /= (float)((double)N * (double)C * (double)S);
    loss[0] = dice + ce;
    loss[1] = dice;
    loss[2] = ce;
}

template <int KIND>
__global__ void dice_ce_finalize_kernel(const float* partial, float* loss, int N, long long S, int C, float snr,
                                        float sdr, float alpha, float beta, int regions) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    loss_triple<KIND>(partial, 4, loss, N, S, C, snr, sdr, alpha, beta, regions);
}

// rows [N][nblk][C*7] -> partial[N][C][4], hard[N][C][3] (optional) and the loss triple, one block, fixed order
template <int KIND>
__global__ __launch_bounds__(256) void dice_ce_rows_finalize_kernel(const float* rows, int nblk, float* partial, float* hard,
                                                                    float* loss, int N, long long S, int C, float snr,
                                                                    float sdr, float alpha, float beta, int regions) {
    __shared__ float tot[8 * 16 * 7];
    const int L = C * 7;
    // thread = (column o, row slot): 256 / L' slots per column add every slot-th row, then the slots are added in order
    for (int n = 0; n < N; ++n) {
        const float* base = rows + (long long)n * nblk * L;
        const int cols = L < 256 ? L : 256, G = 256 / cols;
        __shared__ float fin[256];
        for (int c0 = 0; c0 < L; c0 += cols) {
            const int col = threadIdx.x % cols, rg = threadIdx.x / cols, o = c0 + col;
            float s = 0.f;
            if (o < L && rg < G) {
                // eight rows in flight per thread (the adds stay in row order: same sum); a loop of one load per trip paid the
                // memory latency 36 times over: 20 us for 432 rows per sample
                int b = rg;
                for (; b + 7 * G < nblk; b += 8 * G) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = base[(long long)(b + j * G) * L + o];
#pragma unroll
                    for (int j = 0; j < 8; ++j) s += v[j];
                }
                for (; b < nblk; b += G) s += base[(long long)b * L + o];
            }
            __syncthreads();
            fin[threadIdx.x] = s;
            __syncthreads();
            if (o < L && rg == 0) {
                float t = 0.f;
                for (int g = 0; g < G; ++g) t += fin[g * cols + col];
                tot[n * L + o] = t;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N * L; i += 256) {
        const int n = i / L, o = i % L, c = o / 7, k = o % 7;
        if (k < 4) partial[(n * C + c) * 4 + k] = tot[i];
        else if (hard) hard[(n * C + c) * 3 + (k - 4)] = tot[i];
    }
    if (threadIdx.x == 0 && loss) loss_triple<KIND>(tot, 7, loss, N, S, C, snr, sdr, alpha, beta, regions);
}

// REGIONS: no softmax Jacobian -- d[c] = (d dice / d p_c) * p_c * (1 - p_c) + the BCE / focal term of channel c alone
template <typename T, int CMAX, int KIND, bool REGIONS>
__global__ __launch_bounds__(256) void dice_ce_bwd_kernel(const T* __restrict__ logits, long long ld,
                                                          const void* __restrict__ labels, int label_dtype,
                                                          const float* __restrict__ partial, const float* gscale,
                                                          T* __restrict__ dlogits, long long ldd, int N, long long S,
                                                          int C, float snr, float sdr, float alpha, float beta,
                                                          const msseg_region_masks rm) {
    const long long n = blockIdx.y;
    // per (n, c) constants of d dice / d p (d tversky / d p)
    float ka[CMAX], kb[CMAX];
    const float gs = gscale ? gscale[0] : 1.f;
    const float wd = gs / (float)(N * C);
    // weight of the per-element term: cross-entropy (mean over N*S), or focal / the regions' BCE (mean over N*C*S)
    const float wc = gs / (float)((KIND == KIND_DICE_FOCAL || REGIONS) ? (double)N * (double)C * (double)S
                                                                       : (double)N * (double)S);
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        ka[c] = kb[c] = 0.f;
        if (c < C) {
            const float I = partial[(n * C + c) * 4 + 0], p2 = partial[(n * C + c) * 4 + 1], t = partial[(n * C + c) * 4 + 2];
            if constexpr (KIND == KIND_TVERSKY) {
                // loss = 1 - num / D, D = I + alpha*(P - I) + beta*(T - I) + sdr: d/dp = t * (-1/D + num*(1-alpha-beta)/D^2)
                // + num*alpha/D^2 (p2 is P here)
                const float D = I + alpha * (p2 - I) + beta * (t - I) + sdr, num = I + snr;
                ka[c] = (-1.f / D + num * (1.f - alpha - beta) / (D * D)) * wd;   // multiplies t
                kb[c] = num * alpha / (D * D) * wd;                                // constant in p
            } else {
                const float den = p2 + t + sdr, num = 2.f * I + snr;
                ka[c] = -2.f / den * wd;              // multiplies t
                kb[c] = 2.f * num / (den * den) * wd;  // multiplies p
            }
        }
    }
    const bool vec = ld > 0 && ld * (long long)sizeof(T) == 16 && ldd == ld && C <= DT<T>::EPC &&
                     ((((uintptr_t)logits) | ((uintptr_t)dlogits)) & 15) == 0;
    auto grad = [&](float* x, int lab, float* d) {   // x: logits in, probabilities out; d[c] = d loss / d logit c
        if constexpr (REGIONS) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                d[c] = 0.f;
                if (c < C) {
                    const float t = region_target(rm, c, lab);
                    float p, q, L;
                    sigmoid_parts(x[c], p, q, L);
                    if constexpr (KIND == KIND_TVERSKY) d[c] = (ka[c] * t + kb[c]) * (p * q);
                    else d[c] = (ka[c] * t + kb[c] * p) * (p * q);
                    if constexpr (KIND == KIND_DICE_CE) d[c] += wc * (t > 0.f ? -q : p);   // p - t
                    else if constexpr (KIND == KIND_DICE_FOCAL) d[c] += wc * focal_grad(x[c], t);
                }
            }
            return;
        }
        float raw[CMAX];
        if constexpr (KIND == KIND_DICE_FOCAL) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c) raw[c] = x[c];
        }
        float lse;
        softmax_inplace<CMAX>(x, C, lse);
        float g[CMAX], dot = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            const float t = (lab == c) ? 1.f : 0.f;
            if constexpr (KIND == KIND_TVERSKY) g[c] = (c < C) ? (ka[c] * t + kb[c]) : 0.f;
            else g[c] = (c < C) ? (ka[c] * t + kb[c] * x[c]) : 0.f;
            dot += g[c] * x[c];
        }
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            const float t = (lab == c) ? 1.f : 0.f;
            if constexpr (KIND == KIND_DICE_CE) d[c] = (c < C) ? x[c] * (g[c] - dot) + wc * (x[c] - t) : 0.f;
            else if constexpr (KIND == KIND_TVERSKY) d[c] = (c < C) ? x[c] * (g[c] - dot) : 0.f;
            else d[c] = (c < C) ? x[c] * (g[c] - dot) + wc * focal_grad(raw[c], t) : 0.f;
        }
    };
    const long long stride = (long long)gridDim.x * 256;
    if (vec) {
        // 16-byte rows in and out: one vector load and ONE vector store per voxel (the padding channels are written as zeros
        // in the same store), four voxels per trip with all loads first
        constexpr int EPC = DT<T>::EPC;
        for (long long s = blockIdx.x * 256LL + threadIdx.x; s < S; s += 4 * stride) {
            u32x4_t rows4[4];
            int lab4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long sj = s + j * stride;
                rows4[j] = u32x4_t{0u, 0u, 0u, 0u};
                lab4[j] = 0;
                if (sj < S) {
                    rows4[j] = *(const u32x4_t*)(logits + (n * S + sj) * ld);
                    lab4[j] = load_label(labels, label_dtype, n * S + sj);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long sj = s + j * stride;
                if (sj < S) {
                    float x[CMAX], d[CMAX];
                    unpack_row<T, CMAX>(rows4[j], C, x);
                    grad(x, lab4[j], d);
                    u32x4_t o;
                    if constexpr (sizeof(T) == 2) {
                        bf16x8_t h;
#pragma unroll
                        for (int e = 0; e < EPC; ++e) h[e] = (bf16_t)((e < CMAX && e < C) ? d[e < CMAX ? e : 0] : 0.f);
                        o = __builtin_bit_cast(u32x4_t, h);
                    } else {
                        f32x4_t f;
#pragma unroll
                        for (int e = 0; e < EPC; ++e) f[e] = (e < CMAX && e < C) ? d[e < CMAX ? e : 0] : 0.f;
                        o = __builtin_bit_cast(u32x4_t, f);
                    }
                    *(u32x4_t*)(dlogits + (n * S + sj) * ldd) = o;
                }
            }
        }
        return;
    }
    for (long long s = blockIdx.x * 256LL + threadIdx.x; s < S; s += stride) {
        float x[CMAX], d[CMAX];
        load_logits<T, CMAX>(logits, ld, S, C, n, s, x);
        const int lab = load_label(labels, label_dtype, n * S + s);
        grad(x, lab, d);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c < C) {
                if (ldd > 0) DT<T>::st(dlogits + (n * S + s) * ldd + c, d[c]);
                else DT<T>::st(dlogits + (n * C + c) * S + s, d[c]);
            }
        }
        if (ldd > C) {
            for (int c = C; c < ldd; ++c) DT<T>::st(dlogits + (n * S + s) * ldd + c, 0.f);
        }
    }
}

// ---------------- sliding window ----------------
__global__ void sw_normalize_kernel(float* out, const float* cnt, int C, long long V) {
    const long long total = (long long)C * V;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
        out[i] = out[i] / cnt[i % V];
}

// ---- batched forms: one launch per window batch, window starts in a device-resident table ----------------
// table[j] = (b, z0, y0, x0); b < 0 marks an unused slot (short last batch).
// flips[j] (nullable = 0): bit 0 / 1 / 2 mirrors window j along D / H / W -- window voxel r is volume voxel
// start + (R - 1 - r) on a mirrored axis.  Only the voxel index changes: the window is written in its own order, the
// volume row of a W-mirrored window is read as a descending contiguous run.
template <typename T>
__global__ void sw_gather_batch_kernel(const float* __restrict__ vol, long long vol_bstride, T* __restrict__ win,
                                       long long ldw, const int* __restrict__ table, const int* __restrict__ flips,
                                       int nwin, int C, int VD, int VH, int VW, int RD, int RH, int RW, float cval) {
    const long long R = (long long)RD * RH * RW, V = (long long)VD * VH * VW;
    const int j = blockIdx.y;
    const int b = table[j * 4 + 0];
    if (b < 0) return;
    const int z0 = table[j * 4 + 1], y0 = table[j * 4 + 2], x0 = table[j * 4 + 3];
    const int m = flips ? flips[j] : 0;
    const float* vb = vol + (long long)b * vol_bstride;
    for (long long ri = blockIdx.x * 256LL + threadIdx.x; ri < R; ri += (long long)gridDim.x * 256) {
        const int rx = (int)(ri % RW), ry = (int)((ri / RW) % RH), rz = (int)(ri / ((long long)RW * RH));
        const int z = z0 + ((m & 1) ? RD - 1 - rz : rz), y = y0 + ((m & 2) ? RH - 1 - ry : ry),
                  x = x0 + ((m & 4) ? RW - 1 - rx : rx);
        const bool in = (unsigned)z < (unsigned)VD && (unsigned)y < (unsigned)VH && (unsigned)x < (unsigned)VW;
        const long long v = ((long long)z * VH + y) * VW + x;
        for (int c = 0; c < C; ++c) {
            const float val = in ? vb[c * V + v] : cval;
            if (ldw > 0) DT<T>::st(win + ((long long)j * R + ri) * ldw + c, val);
            else DT<T>::st(win + ((long long)j * C + c) * R + ri, val);
        }
    }
}

// Every output voxel touched by the batch is owned by exactly one thread -- the thread of the FIRST window (in table
// order) that covers it -- which then adds the contributions of all windows of the batch covering that voxel, in
// table order, with the reference's two roundings per window (mul, then add): the same fp32 sequence as
// `out[idx] += imp * seg` executed window after window (/root/reference/engine/utils.py:146-148).
// flips[k] (nullable = 0; bits as in the gather): the logits of window k are read at the mirrored window index, the
// weight at the un-mirrored one -- `imp` lives in volume orientation (an even ROI's Gaussian peaks at R / 2 and is not
// symmetric).  Rows of one start under several masks cover the same voxels; the owner rule needs nothing new for them.
template <typename T, int CMAX>
__global__ __launch_bounds__(256) void sw_blend_batch_kernel(const T* __restrict__ win, long long ldw,
                                                             const float* __restrict__ imp, float* __restrict__ out,
                                                             long long out_bstride, float* __restrict__ cnt,
                                                             long long cnt_bstride, const int* __restrict__ table,
                                                             const int* __restrict__ flips, int nwin, int C, int VD,
                                                             int VH, int VW, int RD, int RH, int RW) {
#pragma clang fp contract(off)
    __shared__ int tab[256 * 4];
    __shared__ int flp[256];
    for (int i = threadIdx.x; i < nwin * 4; i += 256) tab[i] = table[i];
    if ((int)threadIdx.x < nwin) flp[threadIdx.x] = flips ? flips[threadIdx.x] : 0;
    __syncthreads();
    const long long R = (long long)RD * RH * RW, V = (long long)VD * VH * VW;
    const bool vecw = ldw > 0 && ldw * (long long)sizeof(T) == 16 && C <= DT<T>::EPC && (((uintptr_t)win) & 15) == 0;
    const int j = blockIdx.y;
    const int b = tab[j * 4 + 0];
    if (b < 0) return;
    const int z0 = tab[j * 4 + 1], y0 = tab[j * 4 + 2], x0 = tab[j * 4 + 3];
    for (long long ri = blockIdx.x * 256LL + threadIdx.x; ri < R; ri += (long long)gridDim.x * 256) {
        const int rx = (int)(ri % RW), ry = (int)((ri / RW) % RH), rz = (int)(ri / ((long long)RW * RH));
        const int z = z0 + rz, y = y0 + ry, x = x0 + rx;
        bool owner = true;
        for (int k = 0; k < j; ++k) {
            if (tab[k * 4] != b) continue;
            const unsigned dz = (unsigned)(z - tab[k * 4 + 1]), dy = (unsigned)(y - tab[k * 4 + 2]),
                           dx = (unsigned)(x - tab[k * 4 + 3]);
            if (dz < (unsigned)RD && dy < (unsigned)RH && dx < (unsigned)RW) { owner = false; break; }
        }
        if (!owner) continue;
        const long long v = ((long long)z * VH + y) * VW + x;
        float* ob = out + (long long)b * out_bstride;
        float* cb = cnt + (long long)b * cnt_bstride;
        float o[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) o[c] = c < C ? ob[c * V + v] : 0.f;
        float cv = cb[v];
        for (int k = j; k < nwin; ++k) {
            if (tab[k * 4] != b) continue;
            const unsigned dz = (unsigned)(z - tab[k * 4 + 1]), dy = (unsigned)(y - tab[k * 4 + 2]),
                           dx = (unsigned)(x - tab[k * 4 + 3]);
            if (dz >= (unsigned)RD || dy >= (unsigned)RH || dx >= (unsigned)RW) continue;
            const long long pi = ((long long)dz * RH + dy) * RW + dx;
            const float w = imp[pi];
            const int m = flp[k];
            const unsigned sz = (m & 1) ? RD - 1 - dz : dz, sy = (m & 2) ? RH - 1 - dy : dy,
                           sx = (m & 4) ? RW - 1 - dx : dx;
            const long long si = ((long long)sz * RH + sy) * RW + sx;    // the logits' voxel; == pi without a mask
            float vals[CMAX];
            if (vecw) {   // 16-byte logits rows (the networks' channels-last logits): one load per (voxel, window)
                unpack_row<T, CMAX>(*(const u32x4_t*)(win + ((long long)k * R + si) * ldw), C, vals);
            } else {
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    vals[c] = c < C ? (ldw > 0 ? DT<T>::ld(win + ((long long)k * R + si) * ldw + c)
                                               : DT<T>::ld(win + ((long long)k * C + c) * R + si)) : 0.f;
            }
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                if (c < C) {
                    const float prod = w * vals[c];
                    o[c] = o[c] + prod;
                }
            }
            cv = cv + w;
        }
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) ob[c * V + v] = o[c];
        cb[v] = cv;
    }
}

template <typename T, int CMAX>
int launch_blend_batch(const void* win, long long ldw, const float* imp, float* out, long long obs, float* cnt,
                              long long cbs, const int* table, const int* flips, int nwin, int C, int VD, int VH, int VW,
                              int RD, int RH, int RW, hipStream_t st) {
    const long long R = (long long)RD * RH * RW;
    long long gx = ceil_div_ll(R, 256);
    if (gx > 65535) gx = 65535;
    hipLaunchKernelGGL((sw_blend_batch_kernel<T, CMAX>), dim3((unsigned)gx, nwin), dim3(256), 0, st, (const T*)win, ldw,
                       imp, out, obs, cnt, cbs, table, flips, nwin, C, VD, VH, VW, RD, RH, RW);
    MSSEG_CHECK_LAUNCH("sw_blend_batch");
    return MSSEG_OK;
}

// calls f(std::integral_constant<int, KIND>) for a run-time loss kind (checked by the entry points)
template <typename F> void for_kind(int kind, F&& f) {
    if (kind == KIND_TVERSKY) f(std::integral_constant<int, KIND_TVERSKY>{});
    else if (kind == KIND_DICE_FOCAL) f(std::integral_constant<int, KIND_DICE_FOCAL>{});
    else f(std::integral_constant<int, KIND_DICE_CE>{});
}
// ... and f(kind, std::bool_constant<REGIONS>) with the masks to hand to the kernel by value: those at `masks`, or zeros for
// the softmax kinds (masks == nullptr), which do not read them
template <typename F> void for_kind_regions(int kind, const msseg_region_masks* masks, F&& f) {
    const msseg_region_masks rm = masks ? *masks : msseg_region_masks{};
    for_kind(kind, [&](auto k) {
        if (masks) f(k, std::true_type{}, rm);
        else f(k, std::false_type{}, rm);
    });
}

template <typename T, int CMAX>
int launch_partials(const void* logits, long long ld, const void* labels, int label_dtype, float* partial, float* hard,
                    int N, long long S, int C, int kind, const msseg_region_masks* masks, hipStream_t st,
                    float* rows = nullptr, int* nblk_out = nullptr) {
    long long blocks = ceil_div_ll(S, 256LL * 8);
    const long long cap = (long long)msseg_num_cus() * 8 / N + 1;
    if (blocks > cap) blocks = cap;
    const long long vpb = ceil_div_ll(S, blocks);
    blocks = ceil_div_ll(S, vpb);
    if (nblk_out) *nblk_out = (int)blocks;
    for_kind_regions(kind, masks, [&](auto k, auto r, const msseg_region_masks& rm) {
        hipLaunchKernelGGL((dice_ce_partials_kernel<T, CMAX, decltype(k)::value, decltype(r)::value>),
                           dim3((unsigned)blocks, N), dim3(256), 0, st, (const T*)logits, ld, labels, label_dtype, partial,
                           hard, S, C, vpb, rows, rm);
    });
    MSSEG_CHECK_LAUNCH("dice_ce_partials");
    return MSSEG_OK;
}

template <typename T, int CMAX>
int launch_fwd(const void* logits, long long ld, const void* labels, int label_dtype, float* partial, float* hard,
               float* loss, int N, long long S, int C, float snr, float sdr, int kind, float alpha, float beta,
               const msseg_region_masks* masks, float* rows, hipStream_t st) {
    int nblk = 0;
    const int rc = launch_partials<T, CMAX>(logits, ld, labels, label_dtype, partial, hard, N, S, C, kind, masks, st, rows,
                                            &nblk);
    if (rc) return rc;
    for_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(dice_ce_rows_finalize_kernel<decltype(k)::value>, dim3(1), dim3(256), 0, st, rows, nblk, partial,
                           hard, loss, N, S, C, snr, sdr, alpha, beta, masks ? 1 : 0);
    });
    MSSEG_CHECK_LAUNCH("dice_ce_rows_finalize");
    return MSSEG_OK;
}

template <typename T, int CMAX>
int launch_bwd(const void* logits, long long ld, const void* labels, int label_dtype, const float* partial,
               const float* gscale, void* dlogits, long long ldd, int N, long long S, int C, float snr, float sdr, int kind,
               float alpha, float beta, const msseg_region_masks* masks, hipStream_t st) {
    long long blocks = ceil_div_ll(S, 256LL * 4);
    const long long cap = (long long)msseg_num_cus() * 16 / N + 1;
    if (blocks > cap) blocks = cap;
    for_kind_regions(kind, masks, [&](auto k, auto r, const msseg_region_masks& rm) {
        hipLaunchKernelGGL((dice_ce_bwd_kernel<T, CMAX, decltype(k)::value, decltype(r)::value>), dim3((unsigned)blocks, N),
                           dim3(256), 0, st, (const T*)logits, ld, labels, label_dtype, partial, gscale, (T*)dlogits, ldd, N,
                           S, C, snr, sdr, alpha, beta, rm);
    });
    MSSEG_CHECK_LAUNCH("dice_ce_bwd");
    return MSSEG_OK;
}

}  // namespace

#define DISPATCH_TC(dtype, C, FN, ...)                                                        \
    do {                                                                                      \
        int rc__ = MSSEG_OK;                                                                  \
        const bool known__ = for_dtype(dtype, [&](auto t__) {                                 \
            using T_ = typename decltype(t__)::type;                                          \
            rc__ = (C) <= 4 ? FN<T_, 4>(__VA_ARGS__)                                          \
                 : (C) <= 8 ? FN<T_, 8>(__VA_ARGS__) : FN<T_, 16>(__VA_ARGS__);               \
        });                                                                                   \
        if (!known__) MSSEG_FAIL(MSSEG_EINVAL, "bad dtype %d", (int)(dtype));                 \
        return rc__;                                                                          \
    } while (0)

// the bodies of the msseg_seg_loss_* (masks == nullptr) and msseg_region_loss_* entry points
static int loss_partials(const void* logits, long long ld, int dtype, const void* labels, int label_dtype, float* partial,
                         float* hard, int N, long long S, int C, int kind, const msseg_region_masks* masks,
                         msseg_stream_t stream) {
    if (!logits || !labels || (!partial && !hard) || N < 1 || S < 1 || C < 1 || C > 16 || (ld != 0 && ld < C) ||
        label_dtype < 0 || label_dtype > 3 || kind < 0 || kind > 2)
        MSSEG_FAIL(MSSEG_EINVAL, "seg_loss_partials: bad args (C=%d must be 1..16, kind=%d 0..2)", C, kind);
    DISPATCH_TC(dtype, C, launch_partials, logits, ld, labels, label_dtype, partial, hard, N, S, C, kind, masks,
                (hipStream_t)stream);
}

static int loss_fwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype, float* partial,
                    float* hard, float* loss, int N, long long S, int C, float smooth_nr, float smooth_dr, int kind,
                    float alpha, float beta, const msseg_region_masks* masks, void* scratch, size_t scratch_bytes,
                    msseg_stream_t stream) {
    if (!logits || !labels || !partial || !loss || N < 1 || N > 8 || S < 1 || C < 1 || C > 16 || (ld != 0 && ld < C) ||
        label_dtype < 0 || label_dtype > 3 || kind < 0 || kind > 2)
        MSSEG_FAIL(MSSEG_EINVAL, "seg_loss_fwd: bad args (1 <= N <= 8, 1 <= C <= 16, 0 <= kind <= 2)");
    const size_t need = MSSEG_SCRATCH_HEADER_BYTES + (size_t)N * ((size_t)msseg_num_cus() * 8 / N + 2) * C * 7 * 4;
    if (!scratch || ((uintptr_t)scratch & 255) || scratch_bytes < need)
        MSSEG_FAIL(MSSEG_EWORKSPACE, "seg_loss_fwd: scratch of %zu bytes needed", need);
    float* rows = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    DISPATCH_TC(dtype, C, launch_fwd, logits, ld, labels, label_dtype, partial, hard, loss, N, S, C, smooth_nr, smooth_dr,
                kind, alpha, beta, masks, rows, (hipStream_t)stream);
}

static int loss_finalize(const float* partial, float* loss, int N, long long S, int C, float smooth_nr, float smooth_dr,
                         int kind, float alpha, float beta, int regions, msseg_stream_t stream) {
    if (!partial || !loss || N < 1 || S < 1 || C < 1 || kind < 0 || kind > 2)
        MSSEG_FAIL(MSSEG_EINVAL, "seg_loss_finalize: bad args");
    for_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(dice_ce_finalize_kernel<decltype(k)::value>, dim3(1), dim3(64), 0, (hipStream_t)stream, partial,
                           loss, N, S, C, smooth_nr, smooth_dr, alpha, beta, regions);
    });
    MSSEG_CHECK_LAUNCH("seg_loss_finalize");
    return MSSEG_OK;
}

static int loss_bwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype, const float* partial,
                    const float* gscale, void* dlogits, long long ldd, int N, long long S, int C, float smooth_nr,
                    float smooth_dr, int kind, float alpha, float beta, const msseg_region_masks* masks,
                    msseg_stream_t stream) {
    if (!logits || !labels || !partial || !dlogits || N < 1 || S < 1 || C < 1 || C > 16 || (ld != 0 && ld < C) ||
        (ldd != 0 && ldd < C) || label_dtype < 0 || label_dtype > 3 || kind < 0 || kind > 2)
        MSSEG_FAIL(MSSEG_EINVAL, "seg_loss_bwd: bad args");
    DISPATCH_TC(dtype, C, launch_bwd, logits, ld, labels, label_dtype, partial, gscale, dlogits, ldd, N, S, C, smooth_nr,
                smooth_dr, kind, alpha, beta, masks, (hipStream_t)stream);
}

extern "C" {

int msseg_seg_loss_partials(const void* logits, long long ld, int dtype, const void* labels, int label_dtype,
                            float* partial, float* hard, int N, long long S, int C, int kind, msseg_stream_t stream) {
    return loss_partials(logits, ld, dtype, labels, label_dtype, partial, hard, N, S, C, kind, nullptr, stream);
}

int msseg_seg_loss_fwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype, float* partial,
                       float* hard, float* loss, int N, long long S, int C, float smooth_nr, float smooth_dr, int kind,
                       float alpha, float beta, void* scratch, size_t scratch_bytes, msseg_stream_t stream) {
    return loss_fwd(logits, ld, dtype, labels, label_dtype, partial, hard, loss, N, S, C, smooth_nr, smooth_dr, kind, alpha,
                    beta, nullptr, scratch, scratch_bytes, stream);
}

int msseg_seg_loss_finalize(const float* partial, float* loss, int N, long long S, int C, float smooth_nr,
                            float smooth_dr, int kind, float alpha, float beta, msseg_stream_t stream) {
    return loss_finalize(partial, loss, N, S, C, smooth_nr, smooth_dr, kind, alpha, beta, 0, stream);
}

int msseg_seg_loss_bwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype,
                       const float* partial, const float* gscale, void* dlogits, long long ldd, int N, long long S, int C,
                       float smooth_nr, float smooth_dr, int kind, float alpha, float beta, msseg_stream_t stream) {
    return loss_bwd(logits, ld, dtype, labels, label_dtype, partial, gscale, dlogits, ldd, N, S, C, smooth_nr, smooth_dr,
                    kind, alpha, beta, nullptr, stream);
}

// the sigmoid (region) forms: the same passes with the masks; C outside 1..16 is refused before anything is launched
#define REGION_ARGS_OK(who)                                                                                   \
    if (!masks || C < 1 || C > 16) MSSEG_FAIL(MSSEG_EINVAL, who ": needs the region masks and 1 <= C <= 16 (got C=%d)", C)

int msseg_region_loss_partials(const void* logits, long long ld, int dtype, const void* labels, int label_dtype,
                               float* partial, float* hard, int N, long long S, int C, int kind,
                               const msseg_region_masks* masks, msseg_stream_t stream) {
    REGION_ARGS_OK("region_loss_partials");
    return loss_partials(logits, ld, dtype, labels, label_dtype, partial, hard, N, S, C, kind, masks, stream);
}

int msseg_region_loss_fwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype, float* partial,
                          float* hard, float* loss, int N, long long S, int C, float smooth_nr, float smooth_dr, int kind,
                          float alpha, float beta, const msseg_region_masks* masks, void* scratch, size_t scratch_bytes,
                          msseg_stream_t stream) {
    REGION_ARGS_OK("region_loss_fwd");
    return loss_fwd(logits, ld, dtype, labels, label_dtype, partial, hard, loss, N, S, C, smooth_nr, smooth_dr, kind, alpha,
                    beta, masks, scratch, scratch_bytes, stream);
}

int msseg_region_loss_finalize(const float* partial, float* loss, int N, long long S, int C, float smooth_nr,
                               float smooth_dr, int kind, float alpha, float beta, msseg_stream_t stream) {
    if (C < 1 || C > 16) MSSEG_FAIL(MSSEG_EINVAL, "region_loss_finalize: 1 <= C <= 16 (got C=%d)", C);
    return loss_finalize(partial, loss, N, S, C, smooth_nr, smooth_dr, kind, alpha, beta, 1, stream);
}

int msseg_region_loss_bwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype,
                          const float* partial, const float* gscale, void* dlogits, long long ldd, int N, long long S,
                          int C, float smooth_nr, float smooth_dr, int kind, float alpha, float beta,
                          const msseg_region_masks* masks, msseg_stream_t stream) {
    REGION_ARGS_OK("region_loss_bwd");
    return loss_bwd(logits, ld, dtype, labels, label_dtype, partial, gscale, dlogits, ldd, N, S, C, smooth_nr, smooth_dr,
                    kind, alpha, beta, masks, stream);
}

int msseg_sw_normalize(float* out, const float* cnt, int C, long long V, msseg_stream_t stream) {
    if (!out || !cnt || C < 1 || V < 1) MSSEG_FAIL(MSSEG_EINVAL, "sw_normalize: bad args");
    hipLaunchKernelGGL(sw_normalize_kernel, dim3(stream_grid((long long)C * V, 1024)), dim3(256), 0, (hipStream_t)stream, out, cnt,
                       C, V);
    MSSEG_CHECK_LAUNCH("sw_normalize");
    return MSSEG_OK;
}

int msseg_sw_blend_batch(const void* win, long long ldw, int dtype, const float* imp, float* out, long long out_bstride,
                         float* cnt, long long cnt_bstride, const int* table, const int* flips, int nwin, int C, int VD,
                         int VH, int VW, int RD, int RH, int RW, msseg_stream_t stream) {
    if (!win || !imp || !out || !cnt || !table) MSSEG_FAIL(MSSEG_EINVAL, "sw_blend_batch: null pointer");
    if (nwin < 1 || nwin > 256) MSSEG_FAIL(MSSEG_EINVAL, "sw_blend_batch: 1 <= nwin <= 256 windows per launch (got %d)", nwin);
    if (C < 1 || C > 16) MSSEG_FAIL(MSSEG_EINVAL, "sw_blend_batch: 1 <= C <= 16 classes");
    if (RD < 1 || RH < 1 || RW < 1 || RD > VD || RH > VH || RW > VW)
        MSSEG_FAIL(MSSEG_EINVAL, "sw_blend_batch: roi (%d,%d,%d) does not fit the volume (%d,%d,%d)", RD, RH, RW, VD, VH, VW);
    DISPATCH_TC(dtype, C, launch_blend_batch, win, ldw, imp, out, out_bstride, cnt, cnt_bstride, table, flips, nwin, C,
                VD, VH, VW, RD, RH, RW, (hipStream_t)stream);
}

int msseg_sw_gather_batch(const float* vol, long long vol_bstride, void* win, long long ldw, int dtype, const int* table,
                          const int* flips, int nwin, int C, int VD, int VH, int VW, int RD, int RH, int RW, float cval,
                          msseg_stream_t stream) {
    if (!vol || !win || !table) MSSEG_FAIL(MSSEG_EINVAL, "sw_gather_batch: null pointer");
    if (nwin < 1 || nwin > 65535 || C < 1) MSSEG_FAIL(MSSEG_EINVAL, "sw_gather_batch: bad window / channel count");
    if (ldw != 0 && ldw < C) MSSEG_FAIL(MSSEG_EINVAL, "sw_gather_batch: ldw smaller than the channel count");
    const long long R = (long long)RD * RH * RW;
    long long gx = ceil_div_ll(R, 256LL * 2);
    if (gx > 65535) gx = 65535;
    const bool known = for_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(sw_gather_batch_kernel<T>, dim3((unsigned)gx, nwin), dim3(256), 0, (hipStream_t)stream, vol,
                           vol_bstride, (T*)win, ldw, table, flips, nwin, C, VD, VH, VW, RD, RH, RW, cval);
    });
    if (!known) MSSEG_FAIL(MSSEG_EINVAL, "sw_gather_batch: bad dtype");
    MSSEG_CHECK_LAUNCH("sw_gather_batch");
    return MSSEG_OK;
}

}  // extern "C"
