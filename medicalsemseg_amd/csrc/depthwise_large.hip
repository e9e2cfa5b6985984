// Depthwise Conv3d with odd kernels k = 3, 5, 7, 9, 11 (stride 1, pad k/2, groups = channels, no bias) on channels-last
// tensors, gfx950: the two convolutions of every focal modulation block (models/backbones/focalnet_3d.py:73-81 of the
// reference: 9^3 and 11^3 at the defaults).  729 / 1331 MACs per output element and a few bytes of traffic: compute-bound
// VALU stencils, so the input is staged ONCE per tile in LDS and every LDS value is reused from registers across the kw
// taps by sliding along W.
//
//   forward / input gradient : block = (sample, 16-byte channel chunk, 4 x 8 x 8 output tile), 512 threads.  The tile with
//                              its halo and the chunk's k^3 taps (mirrored for the input gradient) sit in LDS.  Thread =
//                              (output row (d, h) of 8 voxels, slice of the k^2 (kd, kh) tap rows): per tap row it reads
//                              the k weights and the 8 + k - 1 input chunks of the row (ds_read_b128) and does 8 k E FMAs.
//                              The 16 slices are added by a fixed tree through LDS.
//   weight gradient          : thread = ((kd, kh) tap row, d plane of the tile) with k x E accumulators that live across
//                              all tiles of the block; x halo and dy tile in LDS; the four d planes are added in order,
//                              blocks leave partial rows [k^3][C] that a second kernel adds in row order (deterministic,
//                              no atomics).
//
// LDS image: row stride WWP chunks (odd) and a plane stride PS with PS = L * WWP (mod 16), L the number of consecutive
// lanes that walk one plane (8 output rows forward, k tap rows in the weight gradient): the 16-byte slot of a lane is then
// lane * WWP (mod 16) and every 16-lane group of a ds_read_b128 (lanes distinct mod 16) touches 16 distinct slots.
#include "common.h"

namespace {

constexpr int TD = 4, TH = 8, TW = 8;     // output tile
constexpr int NR = TD * TH;               // rows of TW outputs
constexpr int NT = 512;
constexpr int NS = NT / NR;               // tap-row slices (forward)

template <int K, int L> struct Geo {
    static constexpr int PAD = K / 2, K3 = K * K * K;
    static constexpr int ZD = TD + K - 1, HH = TH + K - 1, WW = TW + K - 1;
    static constexpr int WWP = WW | 1;
    static constexpr int PS = HH * WWP + ((((L * WWP) & 15) - ((HH * WWP) & 15)) & 15);
    static constexpr int HALO = ZD * PS;  // chunks
};

// unpack of a chunk that is already in registers (the LDS halo reads); memory <-> floats is Chunk<T> of common.h
template <typename T> struct Cv;
template <> struct Cv<bf16_t> {
    static constexpr int E = 8;
    static MSSEG_DEVFN void up(const u32x4_t& v, float* f) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = __builtin_bit_cast(float, v[i] << 16);
            f[2 * i + 1] = __builtin_bit_cast(float, v[i] & 0xffff0000u);
        }
    }
};
template <> struct Cv<float> {
    static constexpr int E = 4;
    static MSSEG_DEVFN void up(const u32x4_t& v, float* f) {
        const f32x4_t fv = __builtin_bit_cast(f32x4_t, v);     // (a bit_cast of the vector ELEMENT v[i] reads element 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = fv[i];
    }
};

struct DwLParams {
    const void* x; long long ldx;
    const void* w;         // [K^3][C] tap-major, compute dtype
    void* y; long long ldy;
    int N, D, H, W, C;
    int flip;
    int tD, tH, tW;        // tiles per axis
};

// the tile's input with its halo -> LDS, zero outside the volume
template <typename T, typename G>
MSSEG_DEVFN void stage_halo(u32x4_t* halo, const T* __restrict__ xg, long long ldx, int n, int d0, int h0, int w0, int D, int H,
                            int W, int c0) {
    for (int i = threadIdx.x; i < G::ZD * G::HH * G::WW; i += NT) {
        const int xw = i % G::WW;
        const int t = i / G::WW;
        const int yh = t % G::HH, zd = t / G::HH;
        const int gd = d0 + zd, gh = h0 + yh, gw = w0 + xw;
        u32x4_t v = {0u, 0u, 0u, 0u};
        if ((unsigned)gd < (unsigned)D && (unsigned)gh < (unsigned)H && (unsigned)gw < (unsigned)W)
            v = *(const u32x4_t*)(xg + ((((long long)n * D + gd) * H + gh) * W + gw) * ldx + c0);
        halo[zd * G::PS + yh * G::WWP + xw] = v;
    }
}

MSSEG_DEVFN void tile_of(long long job, int tD, int tH, int tW, int& n, int& td, int& th, int& tw) {
    tw = (int)(job % tW); job /= tW;
    th = (int)(job % tH); job /= tH;
    td = (int)(job % tD);
    n = (int)(job / tD);
}

template <typename T, int K>
__global__ __launch_bounds__(NT) void dwconvl_fwd_kernel(const DwLParams p) {
    using G = Geo<K, TH>;
    constexpr int E = Cv<T>::E, Q = TW * E / 4, RED = Q * (NS / 2) * NR;
    constexpr int REGION = G::HALO > RED ? G::HALO : RED;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4_t* halo = (u32x4_t*)smem;
    u32x4_t* wl = halo + REGION;
    const int tid = threadIdx.x;
    const int c0 = blockIdx.y * E;
    int n, td, th, tw;
    tile_of(blockIdx.x, p.tD, p.tH, p.tW, n, td, th, tw);
    const T* __restrict__ xg = (const T*)p.x;
    const T* __restrict__ wg = (const T*)p.w;
    stage_halo<T, G>(halo, xg, p.ldx, n, td * TD - G::PAD, th * TH - G::PAD, tw * TW - G::PAD, p.D, p.H, p.W, c0);
    for (int t = tid; t < G::K3; t += NT) wl[t] = *(const u32x4_t*)(wg + (long long)(p.flip ? G::K3 - 1 - t : t) * p.C + c0);
    __syncthreads();

    const int row = tid & (NR - 1), slice = tid / NR;
    const int rd = row / TH, rh = row % TH;
    float acc[TW][E];
#pragma unroll
    for (int o = 0; o < TW; ++o)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[o][e] = 0.f;
    for (int r = slice; r < K * K; r += NS) {
        const int kd = r / K, kh = r - kd * K;
        const u32x4_t* xr = halo + (rd + kd) * G::PS + (rh + kh) * G::WWP;
        const u32x4_t* wr = wl + r * K;
        float wv[K][E];
#pragma unroll
        for (int kw = 0; kw < K; ++kw) Cv<T>::up(wr[kw], wv[kw]);
#pragma unroll
        for (int j = 0; j < TW + K - 1; ++j) {
            float xv[E];
            Cv<T>::up(xr[j], xv);
#pragma unroll
            for (int kw = 0; kw < K; ++kw) {
                const int o = j - kw;
                if (o >= 0 && o < TW) {
#pragma unroll
                    for (int e = 0; e < E; ++e) acc[o][e] = fmaf(xv[e], wv[kw][e], acc[o][e]);
                }
            }
        }
    }
    // slices -> slice 0 by a fixed tree (s += s + half), over the halo's LDS
    __syncthreads();
    f32x4_t* red = (f32x4_t*)smem;
#pragma unroll
    for (int half = NS / 2; half >= 1; half >>= 1) {
        if (slice >= half && slice < 2 * half) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float* a = &acc[0][0] + 4 * q;
                red[(q * (NS / 2) + (slice - half)) * NR + row] = f32x4_t{a[0], a[1], a[2], a[3]};
            }
        }
        __syncthreads();
        if (slice < half) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const f32x4_t v = red[(q * (NS / 2) + slice) * NR + row];
                float* a = &acc[0][0] + 4 * q;
                a[0] += v[0]; a[1] += v[1]; a[2] += v[2]; a[3] += v[3];
            }
        }
        __syncthreads();
    }
    if (slice != 0) return;
    const int gd = td * TD + rd, gh = th * TH + rh;
    if (gd >= p.D || gh >= p.H) return;
    T* __restrict__ yg = (T*)p.y;
    const long long vrow = (((long long)n * p.D + gd) * p.H + gh) * p.W;
#pragma unroll
    for (int o = 0; o < TW; ++o) {
        const int gw = tw * TW + o;
        if (gw < p.W) Chunk<T>::store(yg + (vrow + gw) * p.ldy + c0, acc[o]);
    }
}

struct DwLWgParams {
    const void* x; long long ldx;
    const void* dy; long long lddy;
    float* ws;             // [rows][K^3][C]
    int N, D, H, W, C;
    int tD, tH, tW;
    long long jobs;        // N * tiles
};

constexpr int WG_TR = 128;                // tap-row lanes per d plane (k^2 <= 121 used)

template <typename T, int K>
__global__ __launch_bounds__(NT) void dwconvl_wgrad_kernel(const DwLWgParams p) {
    using G = Geo<K, K>;
    constexpr int E = Cv<T>::E;
    static_assert(K * K <= WG_TR && NT == WG_TR * TD, "thread map");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4_t* halo = (u32x4_t*)smem;
    u32x4_t* dyt = halo + G::HALO;                        // [TD][TH][TW]
    float* red = (float*)(dyt + TD * TH * TW);            // [TD - 1][WG_TR][E]
    const int tid = threadIdx.x;
    const int tr = tid & (WG_TR - 1), g = tid / WG_TR;
    const bool live = tr < K * K;
    const int kd = live ? tr / K : 0, kh = live ? tr - kd * K : 0;
    const int c0 = blockIdx.y * E;
    const T* __restrict__ xg = (const T*)p.x;
    const T* __restrict__ gg = (const T*)p.dy;
    float acc[K][E];
#pragma unroll
    for (int kw = 0; kw < K; ++kw)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[kw][e] = 0.f;
    for (long long job = blockIdx.x; job < p.jobs; job += gridDim.x) {
        int n, td, th, tw;
        tile_of(job, p.tD, p.tH, p.tW, n, td, th, tw);
        __syncthreads();
        stage_halo<T, G>(halo, xg, p.ldx, n, td * TD - G::PAD, th * TH - G::PAD, tw * TW - G::PAD, p.D, p.H, p.W, c0);
        if (tid < TD * TH * TW) {
            const int gd = td * TD + tid / (TH * TW), gh = th * TH + (tid / TW) % TH, gw = tw * TW + tid % TW;
            u32x4_t v = {0u, 0u, 0u, 0u};
            if (gd < p.D && gh < p.H && gw < p.W)
                v = *(const u32x4_t*)(gg + ((((long long)n * p.D + gd) * p.H + gh) * p.W + gw) * p.lddy + c0);
            dyt[tid] = v;
        }
        __syncthreads();
        if (!live || td * TD + g >= p.D) continue;
        const int hn = p.H - th * TH < TH ? p.H - th * TH : TH;
        for (int h = 0; h < hn; ++h) {
            const u32x4_t* xr = halo + (g + kd) * G::PS + (h + kh) * G::WWP;
            const u32x4_t* dr = dyt + (g * TH + h) * TW;
            float dv[TW][E];
#pragma unroll
            for (int o = 0; o < TW; ++o) Cv<T>::up(dr[o], dv[o]);
#pragma unroll
            for (int j = 0; j < TW + K - 1; ++j) {
                float xv[E];
                Cv<T>::up(xr[j], xv);
#pragma unroll
                for (int kw = 0; kw < K; ++kw) {
                    const int o = j - kw;
                    if (o >= 0 && o < TW) {
#pragma unroll
                        for (int e = 0; e < E; ++e) acc[kw][e] = fmaf(xv[e], dv[o][e], acc[kw][e]);
                    }
                }
            }
        }
    }
    // d planes 1..3 -> plane 0 in a fixed order, one kw at a time
    float* row = p.ws + (long long)blockIdx.x * G::K3 * p.C;
#pragma unroll
    for (int kw = 0; kw < K; ++kw) {
        __syncthreads();
        if (g > 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) red[((g - 1) * WG_TR + tr) * E + e] = acc[kw][e];
        }
        __syncthreads();
        if (g == 0 && live) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                float a = acc[kw][e];
#pragma unroll
                for (int s = 0; s < TD - 1; ++s) a += red[(s * WG_TR + tr) * E + e];
                row[(long long)(tr * K + kw) * p.C + c0 + e] = a;
            }
        }
    }
}

// dw[c][tap] (torch layout [C, 1, k, k, k]) (+)= sum over rows, rows added in order by 4 slots that are combined in a fixed
// order (the rule of dwconv3_wgrad_finalize_kernel) -- bit-reproducible
__global__ __launch_bounds__(256) void dwconvl_wgrad_finalize_kernel(const float* ws, int rows, int C, int K3, float* dw, int acc_w) {
    __shared__ float part[4][64];
    const int col = threadIdx.x & 63, slot = threadIdx.x >> 6;
    const long long L = (long long)K3 * C;
    const long long i = (long long)blockIdx.x * 64 + col;     // i = t * C + c
    float s = 0.f;
    if (i < L) {
#pragma unroll 8
        for (int r = slot; r < rows; r += 4) s += ws[(long long)r * L + i];
    }
    part[slot][col] = s;
    __syncthreads();
    if (slot != 0 || i >= L) return;
    s = ((part[0][col] + part[1][col]) + part[2][col]) + part[3][col];
    const long long t = i / C, c = i - t * C;
    float* o = dw + c * K3 + t;
    *o = acc_w ? *o + s : s;
}

int check(const void* x, long long ldx, const void* y, long long ldy, int N, int D, int H, int W, int C, int K, int dtype,
          const char* what) {
    if (!x || !y) MSSEG_FAIL(MSSEG_EINVAL, "%s: null pointer", what);
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "%s: bad dtype", what);
    if (K != 3 && K != 5 && K != 7 && K != 9 && K != 11) MSSEG_FAIL(MSSEG_EINVAL, "%s: kernel size %d (3, 5, 7, 9, 11)", what, K);
    if (N < 1 || D < 1 || H < 1 || W < 1 || C < 1 || C % 8) MSSEG_FAIL(MSSEG_EINVAL, "%s: channels must be a multiple of 8", what);
    if (ldx < C || ldy < C || ldx % 8 || ldy % 8 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15))
        MSSEG_FAIL(MSSEG_EINVAL, "%s: tensors must be 16-byte aligned with voxel strides that are multiples of 8", what);
    if ((long long)N * ceil_div(D, TD) * ceil_div(H, TH) * ceil_div(W, TW) > 0x7fffffffLL)
        MSSEG_FAIL(MSSEG_EINVAL, "%s: volume too large", what);
    return MSSEG_OK;
}

template <typename T, int K>
int launch_fwd(const DwLParams& p, hipStream_t stream) {
    using G = Geo<K, TH>;
    constexpr int E = Cv<T>::E, Q = TW * E / 4, RED = Q * (NS / 2) * NR;
    constexpr int lds = ((G::HALO > RED ? G::HALO : RED) + G::K3) * 16;
    static_assert(lds <= 160 * 1024, "LDS");
    auto kern = dwconvl_fwd_kernel<T, K>;
    static msseg_lds_attr_once attr;
    if (!attr.ensure((const void*)kern, lds)) MSSEG_FAIL(MSSEG_ELAUNCH, "dwconv3d_fwd: cannot set dynamic LDS size %d", lds);
    const dim3 grid((unsigned)(p.N * p.tD * p.tH * p.tW), (unsigned)(p.C / E));
    MSSEG_KTIMED("dwconvl_fwd_kernel", stream, hipLaunchKernelGGL(kern, grid, dim3(NT), lds, stream, p));
    MSSEG_CHECK_LAUNCH("dwconv3d_fwd");
    return MSSEG_OK;
}

template <typename T, int K>
int launch_wgrad(const DwLWgParams& p, int rows, hipStream_t stream) {
    using G = Geo<K, K>;
    constexpr int E = Cv<T>::E;
    constexpr int lds = (G::HALO + TD * TH * TW) * 16 + (TD - 1) * WG_TR * E * 4;
    static_assert(lds <= 160 * 1024, "LDS");
    auto kern = dwconvl_wgrad_kernel<T, K>;
    static msseg_lds_attr_once attr;
    if (!attr.ensure((const void*)kern, lds)) MSSEG_FAIL(MSSEG_ELAUNCH, "dwconv3d_wgrad: cannot set dynamic LDS size %d", lds);
    MSSEG_KTIMED("dwconvl_wgrad_kernel", stream,
                 hipLaunchKernelGGL(kern, dim3((unsigned)rows, (unsigned)(p.C / E)), dim3(NT), lds, stream, p));
    MSSEG_CHECK_LAUNCH("dwconv3d_wgrad");
    return MSSEG_OK;
}

// partial rows a launch uses: enough blocks to fill the chip, never more than there are tiles
long long wgrad_rows(int N, int D, int H, int W, int C, int dtype) {
    const long long jobs = (long long)N * ceil_div(D, TD) * ceil_div(H, TH) * ceil_div(W, TW);
    const int nch = C / epc_of(dtype);
    long long rows = ceil_div(2 * msseg_num_cus(), nch);
    if (rows > jobs) rows = jobs;
    return rows < 1 ? 1 : rows;
}

}  // namespace

extern "C" {

int msseg_dwconv3d_fwd(const void* x, long long ldx, const void* w_taps, void* y, long long ldy, int N, int D, int H, int W,
                       int C, int K, int flip, int dtype, msseg_stream_t stream) {
    int rc = check(x, ldx, y, ldy, N, D, H, W, C, K, dtype, "dwconv3d_fwd");
    if (rc) return rc;
    if (!w_taps || ((uintptr_t)w_taps & 15)) MSSEG_FAIL(MSSEG_EINVAL, "dwconv3d_fwd: weight table must be 16-byte aligned");
    const DwLParams p{x, ldx, w_taps, y, ldy, N, D, H, W, C, flip ? 1 : 0, ceil_div(D, TD), ceil_div(H, TH), ceil_div(W, TW)};
    hipStream_t s = (hipStream_t)stream;
#define DWL_FWD(K_) case K_: return dtype == MSSEG_F32 ? launch_fwd<float, K_>(p, s) : launch_fwd<bf16_t, K_>(p, s)
    switch (K) {
        DWL_FWD(3); DWL_FWD(5); DWL_FWD(7); DWL_FWD(9); DWL_FWD(11);
    }
#undef DWL_FWD
    MSSEG_FAIL(MSSEG_EINVAL, "dwconv3d_fwd: kernel size %d", K);
}

size_t msseg_dwconv3d_wgrad_workspace_bytes(int N, int D, int H, int W, int C, int K, int dtype) {
    if (N < 1 || D < 1 || H < 1 || W < 1 || C < 1 || K < 1) return 0;
    return (size_t)wgrad_rows(N, D, H, W, C, dtype) * K * K * K * C * sizeof(float);
}

int msseg_dwconv3d_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw, int accumulate, int N, int D,
                         int H, int W, int C, int K, void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream) {
    int rc = check(x, ldx, dy, lddy, N, D, H, W, C, K, dtype, "dwconv3d_wgrad");
    if (rc) return rc;
    if (!dw) MSSEG_FAIL(MSSEG_EINVAL, "dwconv3d_wgrad: null pointer");
    const size_t row_bytes = (size_t)K * K * K * C * sizeof(float);
    long long rows = wgrad_rows(N, D, H, W, C, dtype);
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < row_bytes)
        MSSEG_FAIL(MSSEG_EWORKSPACE, "dwconv3d_wgrad: needs a 16-byte aligned workspace of %zu bytes",
                   msseg_dwconv3d_wgrad_workspace_bytes(N, D, H, W, C, K, dtype));
    if ((size_t)rows * row_bytes > workspace_bytes) rows = (long long)(workspace_bytes / row_bytes);   // fewer, longer rows
    const DwLWgParams p{x, ldx, dy, lddy, (float*)workspace, N, D, H, W, C, ceil_div(D, TD), ceil_div(H, TH), ceil_div(W, TW),
                        (long long)N * ceil_div(D, TD) * ceil_div(H, TH) * ceil_div(W, TW)};
    hipStream_t s = (hipStream_t)stream;
#define DWL_WG(K_) case K_: rc = dtype == MSSEG_F32 ? launch_wgrad<float, K_>(p, (int)rows, s) : launch_wgrad<bf16_t, K_>(p, (int)rows, s); break
    switch (K) {
        DWL_WG(3); DWL_WG(5); DWL_WG(7); DWL_WG(9); DWL_WG(11);
    }
#undef DWL_WG
    if (rc) return rc;
    const long long L = (long long)K * K * K * C;
    hipLaunchKernelGGL(dwconvl_wgrad_finalize_kernel, dim3((unsigned)ceil_div_ll(L, 64)), dim3(256), 0, s, (const float*)workspace,
                       (int)rows, C, K * K * K, dw, accumulate);
    MSSEG_CHECK_LAUNCH("dwconv3d_wgrad_finalize");
    return MSSEG_OK;
}

}  // extern "C"
