// Per-volume, per-channel statistics of a cached fp32 volume [C][V] over its non-zero voxels, and the z-score that uses
// them (--t_zscore / --t_zscore_clip; nnU-Net's ZScoreNormalization with use_mask_for_norm, MONAI's
// NormalizeIntensityd(nonzero=True, channel_wise=True) taken per volume).  Semantics: tests/zscore_ref.py.
//
//   select_f32       exact order statistics of the masked values: radix select on the order-preserving 32-bit key, 8 bits per
//                    pass from the top, 4 passes; per-block LDS histograms [rank][256] flushed with integer atomics, a one-wave
//                    step kernel between the passes (the shape of sd_select_* in surface_mm.hip).  The masked count n comes
//                    out of the first pass; with percentages the ranks k, k + 1 are formed from it on the device.
//   masked_moments   n and the sum of the (clipped) masked values, then the sum of their squared deviations from the double
//                    mean: per-block partial rows in double, summed in a fixed order by a finish kernel.
//   zscore_apply     in place: clip + (y - mean) / std on the mask, one fp32 rounding per operation.
//
// The mask is x != 0 (so -0.0 is outside it, a NaN inside).  All kernels are HBM-bound: threads run along the flat voxel
// index in 16-byte vectors, the channel comes from blockIdx.y.  No floating-point atomics: the statistics are bit-identical
// from run to run.
#include <float.h>

#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int VS_MAX_RANK = 4, VS_MAX_PCT = 2, VS_PASSES = 4;
constexpr int VS_MOM_BLOCKS = 1024;                               // partial rows per channel, whatever the device
constexpr int VS_MAX_C = 1024;
constexpr size_t VS_HIST_WORDS = (size_t)VS_PASSES * VS_MAX_RANK * 256;   // u64 per channel
constexpr size_t VS_STATE_WORDS = 32;                                     // u64 per channel, see below
constexpr size_t VS_PART_WORDS = (size_t)VS_MOM_BLOCKS * 4;               // doubles per channel
// state of one channel: [0..3] prefix of each rank's key, [4..7] its remaining rank, [8] n, [10..11] h - floor(h) of each
// percentage (double bits), [12..15] the rank as asked for, [16] the double mean (bits), [17] n as a double (bits)
enum { VS_PREFIX = 0, VS_REMAIN = 4, VS_N = 8, VS_FRAC = 10, VS_ASKED = 12, VS_MEAN = 16, VS_MOM_N = 17 };

struct VsQuery { int nrank, npct; u64 rank[VS_MAX_RANK]; double q01[VS_MAX_PCT]; };

// order-preserving key of an fp32 bit pattern and its inverse
MSSEG_DEVFN unsigned f32_key(float v) {
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
MSSEG_DEVFN float key_f32(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// f(v) for every element of p[0 .. V): 16-byte vectors grid-strided over blockIdx.x, the unaligned head (< 4 elements) and
// the tail (< 4) by block 0; four vectors in flight per thread.  The order in which a thread meets its elements depends on
// V, p's alignment and the grid only.
template <typename F> MSSEG_DEVFN void for_each_of_channel(const float* p, long long V, F&& f) {
    int head = (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u);
    if ((long long)head > V) head = (int)V;
    const long long nvec = (V - head) >> 2;
    const f32x4_t* pv = (const f32x4_t*)(p + head);
    const long long stride = (long long)gridDim.x * 256;
    long long i = blockIdx.x * 256LL + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        f32x4_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = pv[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) { f(v[u][0]); f(v[u][1]); f(v[u][2]); f(v[u][3]); }
    }
    for (; i < nvec; i += stride) {
        const f32x4_t v = pv[i];
        f(v[0]); f(v[1]); f(v[2]); f(v[3]);
    }
    if (blockIdx.x == 0) {
        const long long tail0 = head + nvec * 4;
        const int t = threadIdx.x;
        if (t < head) f(p[t]);
        else if (t >= 64 && tail0 + (t - 64) < V) f(p[tail0 + (t - 64)]);
    }
}
// p[i] = f(p[i]), the same walk
template <typename F> MSSEG_DEVFN void map_channel(float* p, long long V, F&& f) {
    int head = (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u);
    if ((long long)head > V) head = (int)V;
    const long long nvec = (V - head) >> 2;
    f32x4_t* pv = (f32x4_t*)(p + head);
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
        const f32x4_t v = pv[i];
        pv[i] = f32x4_t{f(v[0]), f(v[1]), f(v[2]), f(v[3])};
    }
    if (blockIdx.x == 0) {
        const long long tail0 = head + nvec * 4;
        const int t = threadIdx.x;
        if (t < head) p[t] = f(p[t]);
        else if (t >= 64 && tail0 + (t - 64) < V) p[tail0 + (t - 64)] = f(p[tail0 + (t - 64)]);
    }
}

// ---- select -------------------------------------------------------------------------------------------------------------
__global__ void vs_select_init_kernel(u64* __restrict__ state_all) {
    if (threadIdx.x < VS_MEAN) state_all[(size_t)blockIdx.x * VS_STATE_WORDS + threadIdx.x] = 0ull;   // the select's words
}

// one radix pass: per rank, the histogram of byte (3 - pass) of the key over the masked values whose higher bytes equal the
// rank's prefix.  Ranks that share a prefix share the histogram of the first of them (k and k + 1 mostly do, and in pass 0
// all do); the step kernel reads it from there.
__global__ __launch_bounds__(256) void vs_hist_kernel(const float* __restrict__ x, long long V, int pass, int nrank,
                                                      const u64* __restrict__ state_all, u64* __restrict__ hist_all) {
    __shared__ unsigned int lh[VS_MAX_RANK][256];
    const int c = blockIdx.y;
    const u64* state = state_all + (size_t)c * VS_STATE_WORDS;
    u64* hist = hist_all + ((size_t)c * VS_PASSES + pass) * VS_MAX_RANK * 256;
#pragma unroll
    for (int r = 0; r < VS_MAX_RANK; ++r) lh[r][threadIdx.x] = 0;
    __syncthreads();
    unsigned prefix[VS_MAX_RANK];
    bool lead[VS_MAX_RANK];
#pragma unroll
    for (int r = 0; r < VS_MAX_RANK; ++r) {
        prefix[r] = (unsigned)state[VS_PREFIX + r];
        lead[r] = r < nrank;
#pragma unroll
        for (int e = 0; e < r; ++e) lead[r] = lead[r] && prefix[e] != prefix[r];
    }
    const int shift = 24 - 8 * pass;
    for_each_of_channel(x + (long long)c * V, V, [&](float v) {
        if (v != 0.0f) {
            const unsigned key = f32_key(v);
            const unsigned high = pass ? key >> (shift + 8) : 0u;
            const int digit = (int)((key >> shift) & 255u);
#pragma unroll
            for (int r = 0; r < VS_MAX_RANK; ++r)
                if (lead[r] && high == prefix[r]) atomicAdd(&lh[r][digit], 1u);
        }
    });
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VS_MAX_RANK; ++r)
        if (lead[r] && lh[r][threadIdx.x]) atomicAdd(hist + r * 256 + threadIdx.x, (u64)lh[r][threadIdx.x]);
}

// one wave per channel.  Pass 0 also takes n from the histogram and, with percentages, forms the ranks k = floor(h) and
// min(k + 1, n - 1), h = q / 100 * (n - 1).  Then, per rank, the digit that holds its remaining position; a rank past the
// last entry runs into byte 0xFF on every pass (the finish kernel reports it as NaN).
__global__ void vs_step_kernel(const u64* __restrict__ hist_all, int pass, VsQuery q, u64* __restrict__ state_all) {
#pragma clang fp contract(off)
    const int c = blockIdx.x, r = threadIdx.x;
    u64* state = state_all + (size_t)c * VS_STATE_WORDS;
    const u64* hist = hist_all + ((size_t)c * VS_PASSES + pass) * VS_MAX_RANK * 256;
    u64 old[VS_MAX_RANK];
#pragma unroll
    for (int e = 0; e < VS_MAX_RANK; ++e) old[e] = state[VS_PREFIX + e];
    __syncthreads();
    if (r >= q.nrank) return;
    if (pass == 0) {
        u64 n = 0;
        for (int j = 0; j < 256; ++j) n += hist[j];
        u64 k = q.rank[r < VS_MAX_RANK ? r : 0];
        if (q.npct) {
            const int j = r >> 1;
            const double h = n ? q.q01[j] * (double)(n - 1) : 0.0;
            const double fl = floor(h);
            k = (u64)fl + (u64)(r & 1);
            if (n && k > n - 1) k = n - 1;
            if (!(r & 1)) state[VS_FRAC + j] = (u64)__double_as_longlong(h - fl);
        }
        if (r == 0) state[VS_N] = n;
        state[VS_ASKED + r] = k;
        state[VS_REMAIN + r] = k;
    }
    int lead = r;
    for (int e = r - 1; e >= 0; --e)
        if (old[e] == old[r]) lead = e;
    u64 k = state[VS_REMAIN + r], cum = 0;
    int d = -1;
    for (int j = 0; j < 256; ++j) {
        const u64 cnt = hist[lead * 256 + j];
        if (cum + cnt > k) { d = j; break; }
        cum += cnt;
    }
    if (d < 0) { d = 255; cum = 0; }                             // past the last entry: the remaining rank stays
    state[VS_PREFIX + r] = (old[r] << 8) | (u64)d;
    state[VS_REMAIN + r] = k - cum;
}

// out[c][8] = {n, the nrank order statistics (NaN: rank past the last entry), P_LO, P_HI (-inf, +inf without percentages or
// with an empty mask), 0}
__global__ void vs_select_finish_kernel(const u64* __restrict__ state_all, VsQuery q, double* __restrict__ out_all) {
#pragma clang fp contract(off)
    const int c = blockIdx.x, r = threadIdx.x;
    const u64* state = state_all + (size_t)c * VS_STATE_WORDS;
    double* out = out_all + (size_t)c * 8;
    const u64 n = state[VS_N];
    if (r == 0) { out[0] = (double)n; out[7] = 0.0; }
    if (r < VS_MAX_RANK) {
        const bool valid = r < q.nrank && state[VS_ASKED + r] < n;
        out[1 + r] = valid ? (double)key_f32((unsigned)state[VS_PREFIX + r]) : __builtin_nan("");
    }
    if (r < VS_MAX_PCT) {
        double p = r == 0 ? -__builtin_inf() : __builtin_inf();
        if (r < q.npct && n) {
            const double a = (double)key_f32((unsigned)state[VS_PREFIX + 2 * r]);
            const double b = (double)key_f32((unsigned)state[VS_PREFIX + 2 * r + 1]);
            const double t = __longlong_as_double((long long)state[VS_FRAC + r]);
            p = (double)(float)(a + t * (b - a));
        }
        out[5 + r] = p;
    }
}

// ---- moments ------------------------------------------------------------------------------------------------------------
MSSEG_DEVFN float clip_f32(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

MSSEG_DEVFN double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// PASS 0: row = {sum y, n, number of non-finite masked values, 0}; PASS 1: row = {sum (y - mean)^2, 0, 0, 0}.
// grid (blocks <= VS_MOM_BLOCKS, C): block b of channel c writes row c * VS_MOM_BLOCKS + b
template <int PASS>
__global__ __launch_bounds__(256) void vs_moments_kernel(const float* __restrict__ x, long long V,
                                                         const double* __restrict__ bounds, long long bstride,
                                                         const u64* __restrict__ state_all, double* __restrict__ part_all) {
#pragma clang fp contract(off)
    __shared__ double sm[4][3];
    const int c = blockIdx.y;
    float lo = -__builtin_inff(), hi = __builtin_inff();
    if (bounds) { lo = (float)bounds[(long long)c * bstride]; hi = (float)bounds[(long long)c * bstride + 1]; }
    const double mean = PASS ? __longlong_as_double((long long)state_all[(size_t)c * VS_STATE_WORDS + VS_MEAN]) : 0.0;
    double s = 0.0;
    unsigned cnt = 0, bad = 0;
    for_each_of_channel(x + (long long)c * V, V, [&](float v) {
        if (v != 0.0f) {
            const float y = clip_f32(v, lo, hi);
            if (PASS == 0) {
                s += (double)y;
                ++cnt;
                bad += !(fabsf(v) <= FLT_MAX);
            } else {
                const double d = (double)y - mean;
                s += d * d;
            }
        }
    });
    s = wave_sum_f64(s);
    const double cn = wave_sum_f64((double)cnt), bd = wave_sum_f64((double)bad);
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = s; sm[threadIdx.x >> 6][1] = cn; sm[threadIdx.x >> 6][2] = bd; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        double* row = part_all + ((size_t)c * VS_MOM_BLOCKS + blockIdx.x) * 4;
        row[j] = j < 3 ? ((sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j])) : 0.0;
    }
}

// one block per channel: the nblk rows in a fixed order.  PASS 0: stats[c] = {n, lo, hi, mean, ., non-finite count}, the
// mean also goes to the state; PASS 1: stats[c][4] = the population std, 1 when it is 0 as fp32.  Mean and std stay in
// double here; the apply kernel rounds them once to fp32.
template <int PASS>
__global__ __launch_bounds__(256) void vs_moments_finish_kernel(const double* __restrict__ part_all, int nblk,
                                                                const double* __restrict__ bounds, long long bstride,
                                                                u64* __restrict__ state_all, double* __restrict__ stats_all) {
#pragma clang fp contract(off)
    __shared__ double sm[256][3];
    const int c = blockIdx.x, t = threadIdx.x;
    const double* rows = part_all + (size_t)c * VS_MOM_BLOCKS * 4;
    double a[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < VS_MOM_BLOCKS / 256; ++j) {
        const int b = t * (VS_MOM_BLOCKS / 256) + j;
        if (b < nblk) { a[0] += rows[b * 4 + 0]; a[1] += rows[b * 4 + 1]; a[2] += rows[b * 4 + 2]; }
    }
    sm[t][0] = a[0]; sm[t][1] = a[1]; sm[t][2] = a[2];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { sm[t][0] += sm[t + o][0]; sm[t][1] += sm[t + o][1]; sm[t][2] += sm[t + o][2]; }
        __syncthreads();
    }
    if (t != 0) return;
    u64* state = state_all + (size_t)c * VS_STATE_WORDS;
    double* stats = stats_all + (size_t)c * 6;
    if (PASS == 0) {
        const double n = sm[0][1];
        const double mean = n > 0.0 ? sm[0][0] / n : 0.0;
        state[VS_MEAN] = (u64)__double_as_longlong(mean);
        state[VS_MOM_N] = (u64)__double_as_longlong(n);
        stats[0] = n;
        stats[1] = bounds ? (double)(float)bounds[(long long)c * bstride] : -__builtin_inf();
        stats[2] = bounds ? (double)(float)bounds[(long long)c * bstride + 1] : __builtin_inf();
        stats[3] = mean;
        stats[5] = sm[0][2];
    } else {
        const double n = __longlong_as_double((long long)state[VS_MOM_N]);
        double sd = n > 0.0 ? sqrt(sm[0][0] / n) : 1.0;
        if ((float)sd == 0.0f) sd = 1.0;
        stats[4] = sd;
    }
}

// ---- apply --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vs_apply_kernel(float* __restrict__ x, long long V, const double* __restrict__ stats_all) {
#pragma clang fp contract(off)   // one rounding per numpy operation
    const int c = blockIdx.y;
    const double* stats = stats_all + (size_t)c * 6;
    const float lo = (float)stats[1], hi = (float)stats[2], mean = (float)stats[3], sd = (float)stats[4];
    map_channel(x + (long long)c * V, V, [&](float v) { return v != 0.0f ? (clip_f32(v, lo, hi) - mean) / sd : v; });
}

struct VsScratch { u64* hist; u64* state; double* part; };
inline VsScratch vs_carve(void* scratch, int C) {
    u64* h = (u64*)scratch;
    u64* s = h + (size_t)C * VS_HIST_WORDS;
    return VsScratch{h, s, (double*)(s + (size_t)C * VS_STATE_WORDS)};
}
inline bool vs_dims_ok(const void* x, int C, long long V) {
    return x && !((uintptr_t)x & 15) && C >= 1 && C <= VS_MAX_C && V >= 1 && V < (1LL << 32);
}
// blocks along x of a pass over V voxels in vectors of 4
inline int vs_grid(long long V) { return stream_grid(ceil_div_ll(V, 4)); }
// the same for a histogram pass: at most 8 blocks per CU over all channels, so that a block has enough voxels to
// amortise zeroing its LDS histograms and flushing them with up to 4 x 256 global atomics
inline int vs_hist_grid(long long V, int C) {
    const int cap = msseg_num_cus() * 8 / C, g = vs_grid(V);
    return g < cap ? g : (cap < 1 ? 1 : cap);
}

}  // namespace

extern "C" {

size_t msseg_volume_stats_scratch_bytes(int C) {
    if (C < 1) return 0;
    return (size_t)C * (VS_HIST_WORDS + VS_STATE_WORDS + VS_PART_WORDS) * 8;
}

int msseg_select_f32(const float* x, int C, long long V, const long long* ranks, int nrank, const double* percentages, int npct,
                     void* scratch, size_t scratch_bytes, double* out8, msseg_stream_t stream) {
    if (!vs_dims_ok(x, C, V) || !out8)
        MSSEG_FAIL(MSSEG_EINVAL, "select_f32: bad args (x 16-byte aligned, 1 <= C <= %d, 1 <= V < 2^32)", VS_MAX_C);
    if ((ranks != nullptr) == (percentages != nullptr) || (ranks && (nrank < 1 || nrank > VS_MAX_RANK)) ||
        (percentages && (npct < 1 || npct > VS_MAX_PCT)))
        MSSEG_FAIL(MSSEG_EINVAL, "select_f32: give 1..%d ranks or 1..%d percentages, not both", VS_MAX_RANK, VS_MAX_PCT);
    if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < msseg_volume_stats_scratch_bytes(C))
        MSSEG_FAIL(MSSEG_EWORKSPACE, "select_f32: needs an 8-byte aligned scratch of %zu bytes (got %zu)",
                   msseg_volume_stats_scratch_bytes(C), scratch_bytes);
    VsQuery q{};
    if (ranks) {
        q.nrank = nrank;
        for (int r = 0; r < nrank; ++r) {
            if (ranks[r] < 0) MSSEG_FAIL(MSSEG_EINVAL, "select_f32: rank %d is negative", r);
            q.rank[r] = (u64)ranks[r];
        }
    } else {
        q.npct = npct;
        q.nrank = 2 * npct;
        for (int j = 0; j < npct; ++j) {
            if (!(percentages[j] >= 0.0 && percentages[j] <= 100.0))
                MSSEG_FAIL(MSSEG_EINVAL, "select_f32: percentage %d = %g is outside [0, 100]", j, percentages[j]);
            q.q01[j] = percentages[j] / 100.0;
        }
    }
    const VsScratch ws = vs_carve(scratch, C);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws.hist, 0, (size_t)C * VS_HIST_WORDS * 8, s) != hipSuccess)
        MSSEG_FAIL(MSSEG_ELAUNCH, "select_f32: memset failed");
    hipLaunchKernelGGL(vs_select_init_kernel, dim3(C), dim3(64), 0, s, ws.state);
    const dim3 grid((unsigned)vs_hist_grid(V, C), (unsigned)C);
    for (int p = 0; p < VS_PASSES; ++p) {
        hipLaunchKernelGGL(vs_hist_kernel, grid, dim3(256), 0, s, x, V, p, p == 0 ? 1 : q.nrank, ws.state, ws.hist);
        hipLaunchKernelGGL(vs_step_kernel, dim3(C), dim3(64), 0, s, ws.hist, p, q, ws.state);
    }
    hipLaunchKernelGGL(vs_select_finish_kernel, dim3(C), dim3(64), 0, s, ws.state, q, out8);
    MSSEG_CHECK_LAUNCH("select_f32");
    return MSSEG_OK;
}

int msseg_masked_moments(const float* x, int C, long long V, const double* bounds, long long bound_stride, void* scratch,
                         size_t scratch_bytes, double* stats6, msseg_stream_t stream) {
    if (!vs_dims_ok(x, C, V) || !stats6 || (bounds && bound_stride < 2))
        MSSEG_FAIL(MSSEG_EINVAL, "masked_moments: bad args (x 16-byte aligned, 1 <= C <= %d, 1 <= V < 2^32, bound stride >= 2)",
                   VS_MAX_C);
    if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < msseg_volume_stats_scratch_bytes(C))
        MSSEG_FAIL(MSSEG_EWORKSPACE, "masked_moments: needs an 8-byte aligned scratch of %zu bytes (got %zu)",
                   msseg_volume_stats_scratch_bytes(C), scratch_bytes);
    const VsScratch ws = vs_carve(scratch, C);
    hipStream_t s = (hipStream_t)stream;
    int nblk = vs_grid(V);
    if (nblk > VS_MOM_BLOCKS) nblk = VS_MOM_BLOCKS;
    const dim3 grid((unsigned)nblk, (unsigned)C);
    hipLaunchKernelGGL(vs_moments_kernel<0>, grid, dim3(256), 0, s, x, V, bounds, bound_stride, ws.state, ws.part);
    hipLaunchKernelGGL(vs_moments_finish_kernel<0>, dim3(C), dim3(256), 0, s, ws.part, nblk, bounds, bound_stride, ws.state, stats6);
    hipLaunchKernelGGL(vs_moments_kernel<1>, grid, dim3(256), 0, s, x, V, bounds, bound_stride, ws.state, ws.part);
    hipLaunchKernelGGL(vs_moments_finish_kernel<1>, dim3(C), dim3(256), 0, s, ws.part, nblk, bounds, bound_stride, ws.state, stats6);
    MSSEG_CHECK_LAUNCH("masked_moments");
    return MSSEG_OK;
}

int msseg_zscore_apply(float* x, int C, long long V, const double* stats6, msseg_stream_t stream) {
    if (!vs_dims_ok(x, C, V) || !stats6)
        MSSEG_FAIL(MSSEG_EINVAL, "zscore_apply: bad args (x 16-byte aligned, 1 <= C <= %d, 1 <= V < 2^32)", VS_MAX_C);
    hipLaunchKernelGGL(vs_apply_kernel, dim3((unsigned)vs_grid(V), (unsigned)C), dim3(256), 0, (hipStream_t)stream, x, V, stats6);
    MSSEG_CHECK_LAUNCH("zscore_apply");
    return MSSEG_OK;
}

}  // extern "C"
