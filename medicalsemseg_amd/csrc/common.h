// Common device helpers for the msseg HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/msseg.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;

#define MSSEG_DEVFN __device__ __forceinline__

// ---- error plumbing -------------------------------------------------------------
void msseg_set_error(const char* fmt, ...);
#define MSSEG_FAIL(code, ...)           \
    do {                                \
        msseg_set_error(__VA_ARGS__);   \
        return (code);                  \
    } while (0)
#define MSSEG_CHECK_LAUNCH(name)                                              \
    do {                                                                      \
        hipError_t e__ = hipGetLastError();                                   \
        if (e__ != hipSuccess) MSSEG_FAIL(MSSEG_ELAUNCH, "%s: %s", name, hipGetErrorString(e__)); \
    } while (0)

// ---- optional event pair around ONE kernel launch (ktimer.hip; bench.py's per-kernel roofline) -------
bool msseg_ktimer_on();
int msseg_ktimer_begin(const char* name, hipStream_t stream);
void msseg_ktimer_end(int slot, hipStream_t stream);
#define MSSEG_KTIMED(name, stream, launch_stmt)                               \
    do {                                                                      \
        const int kt__ = msseg_ktimer_on() ? msseg_ktimer_begin(name, stream) : -1; \
        launch_stmt;                                                          \
        if (kt__ >= 0) msseg_ktimer_end(kt__, stream);                        \
    } while (0)

// ---- dynamic LDS above 64 KB ---------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of a (kernel, device) pair.  One of these lives as a
// function-local static next to each kernel instantiation: a bit per device ordinal, set after the first successful
// call on that device; two threads racing on the first call both make the same (idempotent) setting.
#include <atomic>
struct msseg_lds_attr_once {
    std::atomic<unsigned long long> done{0};
    bool ensure(const void* kern, int bytes) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return false;
        const bool tracked = dev >= 0 && dev < 64;
        if (tracked && ((done.load(std::memory_order_acquire) >> dev) & 1ull)) return true;
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
        if (tracked) done.fetch_or(1ull << dev, std::memory_order_release);
        return true;
    }
};

// ---- per-dtype traits -------------------------------------------------------------
// A "chunk" is 16 bytes of consecutive channels: 8 bf16 or 4 f32.  One MFMA k-group
// (4 lane-quarters x 1 chunk) therefore spans CB = 4*EPC channels: 32 (bf16) / 16 (f32).
template <typename T> struct DT;
template <> struct DT<float> {
    static constexpr int EPC = 4;
    static constexpr int CODE = MSSEG_F32;
    static MSSEG_DEVFN float ld(const float* p) { return *p; }
    static MSSEG_DEVFN void st(float* p, float v) { *p = v; }
};
template <> struct DT<bf16_t> {
    static constexpr int EPC = 8;
    static constexpr int CODE = MSSEG_BF16;
    static MSSEG_DEVFN float ld(const bf16_t* p) { return (float)*p; }
    static MSSEG_DEVFN void st(bf16_t* p, float v) { *p = (bf16_t)v; }
};

// D[row = A-row (l>>4)*4+reg][col = B-col l&15] += A[row][k] * B[k][col] over one 16-byte chunk
// per lane-quarter: 32 k (bf16, one 16x16x32 MFMA) or 16 k (f32, four 16x16x4 MFMAs whose
// k-order is permuted identically on both operands).
template <typename T> MSSEG_DEVFN void mma_chunk(f32x4_t& acc, const u32x4_t& a, const u32x4_t& b);
template <> MSSEG_DEVFN void mma_chunk<bf16_t>(f32x4_t& acc, const u32x4_t& a, const u32x4_t& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                  acc, 0, 0, 0);
}
template <> MSSEG_DEVFN void mma_chunk<float>(f32x4_t& acc, const u32x4_t& a, const u32x4_t& b) {
    f32x4_t af = __builtin_bit_cast(f32x4_t, a), bf = __builtin_bit_cast(f32x4_t, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], bf[j], acc, 0, 0, 0);
}

// ---- operand fetches shared by the MFMA kernels ------------------------------------------------------
MSSEG_DEVFN u32x4_t ldg16(const void* p) { return *(const u32x4_t*)p; }

// byte offset, in a bf16 msseg_pack_weights image (T = 1) with nkb k-blocks and cout block width cb, of the 16-byte piece that
// lane quarter q holds of image row `row` of cout block blk in k-block kb: a lane's A fragment for mma_chunk<bf16_t>
MSSEG_DEVFN long long wimg_frag_off(int blk, int nkb, int kb, int q, int cb, int row) {
    return ((((long long)blk * nkb + kb) * 4 + q) * cb + row) * 16;
}
MSSEG_DEVFN long long wimg_kblock_bytes(int cb) { return (long long)4 * cb * 16; }   // from a fragment to the next k-block's

// transposing LDS reads (memory holds rows of the contraction index, 16-bit elements): two of them make the fragment of a
// 32-deep k-step for one 16-channel tile; r0 / r1 are the byte offsets of the lane's two rows from base
MSSEG_DEVFN bf16x4_t lds_tr_read(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) bf16x4_t*)(uintptr_t)(uint32_t)(uintptr_t)p);
}
MSSEG_DEVFN u32x4_t tr_frag(const unsigned char* base, int r0, int r1) {
    const bf16x4_t lo = lds_tr_read(base + r0), hi = lds_tr_read(base + r1);
    const bf16x8_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(u32x4_t, f);
}

// bf16 operands a [.., lda >= ca] and b [.., ldb >= cb] that 16-byte vector accesses can walk row by row
static inline bool msseg_aligned_bf16(int dtype, const void* a, long long lda, int ca, const void* b, long long ldb, int cb) {
    return dtype == MSSEG_BF16 && !((lda % 8) || (ldb % 8) || ((uintptr_t)a & 15) || ((uintptr_t)b & 15) || lda < ca || ldb < cb);
}

// ---- the streaming kernels' accesses: channels as floats in registers -------------------------------------
// one 16-byte chunk at p (16-byte aligned) <-> DT<T>::EPC floats
template <typename T> struct Chunk;
template <> struct Chunk<bf16_t> {
    static constexpr int E = 8;
    static MSSEG_DEVFN void load(const bf16_t* p, float* f) {
        const bf16x8_t v = *(const bf16x8_t*)p;
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
    }
    static MSSEG_DEVFN void unpack(const u32x4_t& raw, float* f) {   // a chunk fetched with ldg16 and kept as loaded
        const bf16x8_t v = __builtin_bit_cast(bf16x8_t, raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
    }
    static MSSEG_DEVFN void store(bf16_t* p, const float* f) {
        bf16x8_t v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (bf16_t)f[e];
        *(bf16x8_t*)p = v;
    }
};
template <> struct Chunk<float> {
    static constexpr int E = 4;
    static MSSEG_DEVFN void load(const float* p, float* f) {
        const f32x4_t v = *(const f32x4_t*)p;
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = v[e];
    }
    static MSSEG_DEVFN void unpack(const u32x4_t& raw, float* f) {
        const f32x4_t v = __builtin_bit_cast(f32x4_t, raw);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = v[e];
    }
    static MSSEG_DEVFN void store(float* p, const float* f) { *(f32x4_t*)p = f32x4_t{f[0], f[1], f[2], f[3]}; }
};

// the 16 bytes Chunk<bf16_t>::store writes, in registers (for a kernel that keeps the chunk in LDS)
MSSEG_DEVFN u32x4_t chunk_pack_bf16(const float* f) {
    bf16x8_t v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16_t)f[e];
    return __builtin_bit_cast(u32x4_t, v);
}

// ---- InstanceNorm + LeakyReLU backward, per element -------------------------------------------------------------------
// Shared by the backward apply pass (instnorm.hip) and by the kernels that apply it to an operand as they load it
// (stem_conv.hip), which must give the apply pass's bits.  The expressions are written as the apply pass has always had them
// and the contraction is the compiler's: in both places it makes one fma of the pre-activation, one of dz - k0 - xh * k1,
// fma(-mean, mean, s2 / S) of the variance and fma(-mean, sc, beta) of the shift (read from the device assembly; writing the
// fmas out changes nothing in the arithmetic but reschedules the apply pass).  tests/test_gpu_inbwd_fused.py compares the bits.
MSSEG_DEVFN void mean_rstd(const float* stats, int n, int C, int c, long long S, float eps, float& mean, float& rstd) {
    const float inv = 1.0f / (float)S;
    const float s = stats[((long long)n * C + c) * 2 + 0], s2 = stats[((long long)n * C + c) * 2 + 1];
    mean = s * inv;
    float var = s2 * inv - mean * mean;
    var = var > 0.f ? var : 0.f;
    rstd = rsqrtf(var + eps);
}
// scale and shift of the normalisation: y = x * sc + sh
MSSEG_DEVFN void norm_scale_shift(const float* gamma, const float* beta, int c, float mean, float rstd, float& sc, float& sh) {
    sc = rstd * (gamma ? gamma[c] : 1.f);
    sh = (beta ? beta[c] : 0.f) - mean * sc;
}
// sign source of the activation where it was not stored: the pre-activation as the forward formed it
MSSEG_DEVFN float norm_preact(float x, float sc, float sh) { return x * sc + sh; }
// the gradient of the pre-activation from the gradient dv of the activation (yv: the activation, or the pre-activation)
MSSEG_DEVFN float norm_bwd_dz(float yv, float dv, float slope) { return yv > 0.f ? dv : dv * slope; }
// the gradient of the raw element x; k0 / k1 = the sample's channel sums of dz and dz * xhat over the voxels, divided by S
MSSEG_DEVFN float norm_bwd_dx(float x, float dz, float mean, float rstd, float sc, float k0, float k1) {
    const float xh = (x - mean) * rstd;
    return sc * (dz - k0 - xh * k1);
}

// input gradient of the <= 4-class 1x1x1 head for channel e of a chunk, rounded to T as the head's backward stores it:
// dl = the voxel's class gradients, wv[k][e] = the weight of class k as T (0 past the last class)
template <typename T, int W> MSSEG_DEVFN float head_da(const float* dl, const float (*wv)[W], int e) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += dl[k] * wv[k][e];
    return (float)(T)acc;
}

// 4 consecutive channels at p (aligned to 4 elements) <-> 4 floats
template <typename T> MSSEG_DEVFN void load4(const T* p, float* f);
template <> MSSEG_DEVFN void load4<float>(const float* p, float* f) { Chunk<float>::load(p, f); }
template <> MSSEG_DEVFN void load4<bf16_t>(const bf16_t* p, float* f) {
    const bf16x4_t v = *(const bf16x4_t*)p;
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = (float)v[e];
}
template <typename T> MSSEG_DEVFN void store4(T* p, const float* f);
template <> MSSEG_DEVFN void store4<float>(float* p, const float* f) { Chunk<float>::store(p, f); }
template <> MSSEG_DEVFN void store4<bf16_t>(bf16_t* p, const float* f) {
    *(bf16x4_t*)p = bf16x4_t{(bf16_t)f[0], (bf16_t)f[1], (bf16_t)f[2], (bf16_t)f[3]};
}

MSSEG_DEVFN float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Fixed-order sum of R partial rows of L floats (L % 4 == 0, L <= 4 * NT) by one block of NT threads: float4-wide,
// every thread with up to 8 independent loads in flight, row slots then combined through LDS in a fixed order
// (bit-reproducible).  The L totals end up in lds[NT * 4 ..]; lds: >= NT * 4 + L floats, 16-byte aligned.
template <int NT>
MSSEG_DEVFN void block_rows_sum(const float* rows, int R, int L, float* lds, long long stride = 0) {
    // stride: distance between rows in floats (a multiple of 4; 0 = L): sums an L-wide column slice of wider rows
    const int tid = threadIdx.x, q = L >> 2;
    const int SL = NT / q;
    const int c4 = tid % q, slot = tid / q;
    const long long q_stride = (stride ? stride : (long long)L) >> 2;
    f32x4_t* l4 = (f32x4_t*)lds;
    if (slot < SL) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        const f32x4_t* src = (const f32x4_t*)rows + c4;
#pragma unroll 8
        for (int x = slot; x < R; x += SL) acc += src[(long long)x * q_stride];
        l4[slot * q + c4] = acc;
    }
    __syncthreads();
    if (tid < q) {
        f32x4_t t = {0.f, 0.f, 0.f, 0.f};
        for (int sl = 0; sl < SL; ++sl) t += l4[sl * q + tid];
        l4[NT + tid] = t;
    }
    __syncthreads();
}

#define MSSEG_SCRATCH_HEADER_BYTES 256
#define MSSEG_STATS_NMAX 8

// the reduce scratch that the two-launch reductions work in: a reserved header (neither read nor written), then the
// partial rows, which a second launch on the same stream adds in a fixed order
static inline int scratch_ok(const void* scratch, size_t bytes, const char* who) {
    if (!scratch || ((uintptr_t)scratch & 255) || bytes < msseg_reduce_scratch_bytes())
        MSSEG_FAIL(MSSEG_EWORKSPACE, "%s: needs a 256-byte aligned scratch of %zu bytes", who,
                   msseg_reduce_scratch_bytes());
    return MSSEG_OK;
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline long long ceil_div_ll(long long a, long long b) { return (a + b - 1) / b; }

// ---- host side of the streaming launches ------------------------------------------------------------------
// grid of a grid-stride launch over `items`, a block taking items_per_block per pass: enough blocks for one pass, at most
// 16 per CU, at least one
static inline int stream_grid(long long items, long long items_per_block = 256) {
    long long b = ceil_div_ll(items, items_per_block);
    const long long cap = (long long)msseg_num_cus() * 16;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

// elements of a 16-byte chunk for a run-time dtype code (DT<T>::EPC)
static inline int epc_of(int dtype) { return dtype == MSSEG_F32 ? 4 : 8; }

// calls f(type_tag<T>{}) with T = float / bf16_t for a run-time dtype code, so that a templated launch is written once:
//   for_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type; hipLaunchKernelGGL(kernel<T>, ...); });
// false, and f not called, for any other code
template <typename T> struct type_tag { using type = T; };
template <typename F> static inline bool for_dtype(int dtype, F&& f) {
    if (dtype == MSSEG_F32) f(type_tag<float>{});
    else if (dtype == MSSEG_BF16) f(type_tag<bf16_t>{});
    else return false;
    return true;
}
// what an entry point returns then
static inline int bad_dtype(int dtype) { MSSEG_FAIL(MSSEG_EINVAL, "bad dtype %d", dtype); }
