// Channel statistics and channel sums (HBM-bound, one pass over the tensor), and the second launch that finishes every
// channel reduction of the library: blocks write partial rows into the reduce scratch, channels_finalize_kernel adds them.
#include "channel_reduce.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// channel statistics: stats[n][c][0..1] += (sum x, sum x^2)
// ---------------------------------------------------------------------------------------------------------
// Finalise per-channel reductions in the last block: `nper` values per (n, c); partials laid out
// ws[(n * nblk + b) * C * nper + c * nper + k].  MODE_OUT 0: out[n][c][k] = sum_b (statistics);
// 1: out[c] (+)= sum_{n,b} (channel sums); 2: red[n][c][k] = sum_b and dparam_k[c] (+)= sum_n red[n][c][k].
MSSEG_DEVFN void finalize_channels(const float* ws, int N, int nblk, int C, int nper, int mode, float* out,
                                   float* dp0, float* dp1, int accumulate) {
    // partial matrix: rows (n, b), L = C*nper floats per row.  Threads tile [row group][column]; every thread keeps
    // UNR loads in flight; row groups are then added in a fixed order through LDS (bit-reproducible).
    __shared__ float fin[256];
    const int L = C * nper;
    const int cols = L < 256 ? L : 256;
    const int G = 256 / cols;               // row groups
    const int col = threadIdx.x % cols, rg = threadIdx.x / cols;
    const bool in256 = threadIdx.x < 256;   // blocks may be larger than the 256 threads this routine tiles
    // blocks split the columns (and, where the samples stay separate -- mode 0 -- the samples over grid.y): with one block
    // a 768-channel statistics row (L = 1536) took six sequential passes per sample
    const int n_step = mode == 0 ? (int)gridDim.y : 1, n_first = mode == 0 ? (int)blockIdx.y : 0;
    for (int c0 = blockIdx.x * cols; c0 < L; c0 += gridDim.x * cols) {
        const int o = c0 + col;
        const bool ok = in256 && o < L && rg < G;
        float tot = 0.f;
        for (int n = n_first; n < N; n += n_step) {
            float s = 0.f;
            if (ok) {
                const float* src = ws + (long long)n * nblk * L + o;
#pragma unroll 16
                for (int bb = rg; bb < nblk; bb += G) s += src[(long long)bb * L];
            }
            __syncthreads();
            if (in256) fin[threadIdx.x] = s;
            __syncthreads();
            if (ok && rg == 0) {
                float t = 0.f;
                for (int g = 0; g < G; ++g) t += fin[g * cols + col];
                if (mode != 1) out[(long long)n * L + o] = t;
                tot += t;
            }
        }
        if (ok && rg == 0) {
            if (mode == 1) {
                out[o] = accumulate ? out[o] + tot : tot;
            } else if (mode == 2) {
                const int c = o / nper, k = o % nper;
                float* dp = (k == 0) ? dp0 : dp1;
                if (dp) dp[c] = accumulate ? dp[c] + tot : tot;
            }
        }
    }
}

__global__ __launch_bounds__(256) void channels_finalize_kernel(const FinalizeArgs a) {
    finalize_channels(a.ws, a.N, a.nblk, a.C, a.nper, a.mode, a.out, a.dp0, a.dp1, a.accumulate);
}

static inline dim3 channels_finalize_grid(const FinalizeArgs& a) {
    const int L = a.C * a.nper;
    int gx = (L + 255) / 256;
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, a.mode == 0 ? (unsigned)(a.N < 1 ? 1 : a.N) : 1u);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(RED_THREADS) void channel_stats_kernel(const T* __restrict__ x, long long ldx, float* out,
                                                            long long S, int C, int groups, int rows_par,
                                                            long long rows_per_block, int nacc, int accumulate,
                                                            float* ws) {
    constexpr int W = VEC ? DT<T>::EPC : 1;
    __shared__ float red[RED_THREADS * 2 * (VEC ? DT<T>::EPC : 1)];
    const int n = blockIdx.y;
    const int g = threadIdx.x % groups, rl = threadIdx.x / groups;
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    long long r1 = r0 + rows_per_block;
    if (r1 > S) r1 = S;
    const T* xn = x + (long long)n * S * ldx;
    float* wsb = ws + ((long long)n * gridDim.x + blockIdx.x) * C * nacc;
    for (int gbase = 0; gbase * W < C; gbase += groups) {   // uniform trip count: barriers inside
        const int gg = gbase + g;
        const bool act = gg * W < C;
        float s[W], s2[W];
#pragma unroll
        for (int e = 0; e < W; ++e) s[e] = s2[e] = 0.f;
        if (act && rl < rows_par) {
#pragma unroll 8
            for (long long r = r0 + rl; r < r1; r += rows_par) {
                if constexpr (VEC) {
                    ChunkV<T> c;
                    c.load(xn + r * ldx + gg * W);
#pragma unroll
                    for (int e = 0; e < W; ++e) { s[e] += c.v[e]; s2[e] += c.v[e] * c.v[e]; }
                } else {
                    const float v = DT<T>::ld(xn + r * ldx + gg);
                    s[0] += v; s2[0] += v * v;
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
        block_rows_reduce<W>(red, groups, rows_par, g, rl, act);
        if (act && rl == 0) {
            const int kmax = rows_par < RED_STAGE2 ? rows_par : RED_STAGE2;
#pragma unroll
            for (int e = 0; e < W; ++e) {
                float a = 0.f, b = 0.f;
                for (int k = 0; k < kmax; ++k) {
                    a += red[((k * groups + g) * W + e) * 2 + 0];
                    b += red[((k * groups + g) * W + e) * 2 + 1];
                }
                const int c = gg * W + e;
                wsb[c * nacc + 0] = a;
                if (nacc == 2) wsb[c * nacc + 1] = b;
            }
        }
    }
}

template <typename T>
int launch_stats(const void* x, long long ldx, float* out, int N, long long S, int C, int nacc, int accumulate,
                 void* scratch, hipStream_t st) {
    const bool vec = vec_ok(x, ldx, C, sizeof(T));
    const RowMap m = row_map(C, vec ? DT<T>::EPC : 1, RED_THREADS);
    long long blocks = reduce_blocks(S, m.rows_par, N, C, nacc);
    const long long rpb = ceil_div_ll(S, blocks);
    blocks = ceil_div_ll(S, rpb);
    dim3 grid((unsigned)blocks, N);
    float* ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    if (vec)
        hipLaunchKernelGGL((channel_stats_kernel<T, true>), grid, dim3(RED_THREADS), 0, st, (const T*)x, ldx, out, S, C,
                           m.groups, m.rows_par, rpb, nacc, accumulate, ws);
    else
        hipLaunchKernelGGL((channel_stats_kernel<T, false>), grid, dim3(RED_THREADS), 0, st, (const T*)x, ldx, out, S, C,
                           m.groups, m.rows_par, rpb, nacc, accumulate, ws);
    MSSEG_CHECK_LAUNCH("channel_stats");
    return msseg_channels_finalize_launch({ws, N, (int)blocks, C, nacc, nacc == 2 ? 0 : 1, out, nullptr, nullptr, accumulate}, st);
}

}  // namespace

int msseg_channels_finalize_launch(const FinalizeArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(channels_finalize_kernel, channels_finalize_grid(a), dim3(256), 0, st, a);
    MSSEG_CHECK_LAUNCH("channels_finalize");
    return MSSEG_OK;
}

extern "C" {

int msseg_channel_stats(const void* x, long long ldx, float* stats, int N, long long S, int C, void* scratch,
                        size_t scratch_bytes, int dtype, msseg_stream_t stream) {
    if (!x || !stats || N < 1 || S < 1 || C < 1 || ldx < C) MSSEG_FAIL(MSSEG_EINVAL, "channel_stats: bad args");
    if (int rc = scratch_ok(scratch, scratch_bytes, "channel_stats")) return rc;
    int rc = MSSEG_OK;
    const bool known = for_dtype(dtype, [&](auto t) {
        rc = launch_stats<typename decltype(t)::type>(x, ldx, stats, N, S, C, 2, 0, scratch, (hipStream_t)stream);
    });
    return known ? rc : bad_dtype(dtype);
}

int msseg_channel_sum(const void* x, long long ldx, float* out, long long rows, int C, int accumulate, void* scratch,
                      size_t scratch_bytes, int dtype, msseg_stream_t stream) {
    if (!x || !out || rows < 1 || C < 1 || ldx < C) MSSEG_FAIL(MSSEG_EINVAL, "channel_sum: bad args");
    if (int rc = scratch_ok(scratch, scratch_bytes, "channel_sum")) return rc;
    int rc = MSSEG_OK;
    const bool known = for_dtype(dtype, [&](auto t) {
        rc = launch_stats<typename decltype(t)::type>(x, ldx, out, 1, rows, C, 1, accumulate, scratch, (hipStream_t)stream);
    });
    return known ? rc : bad_dtype(dtype);
}

}  // extern "C"
