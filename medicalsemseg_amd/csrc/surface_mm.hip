// Surface distances in millimetres on an anisotropic grid, for the scorer of native-grid maps (metrics.surface_metrics:
// HD percentile, average symmetric surface distance, normalised surface Dice as MONAI's compute_hausdorff_distance,
// compute_average_surface_distance(symmetric=True) and compute_surface_dice define them).  Surfaces, the class's box and the
// surface sizes come from hd_edges (hausdorff.hip) unchanged.
//
//   sd_directed_mm  exact squared Euclidean distance in physical units from every class-c surface voxel of map A to the
//                   nearest class-c surface voxel of map B inside the class's box, with one spacing per axis: the separable
//                   minimum min_z' min_y' min_x' (sx (x-x'))^2 + (sy (y-y'))^2 + (sz (z-z'))^2 as hausdorff.hip's three line
//                   passes (x: the shared integer two-sided scan; y and z: outward search that stops once the axis term
//                   (s k)^2 alone reaches the best value), in double with contraction off: every product and sum rounds
//                   once, in the stated order ((x term + y term) + z term).  Output: a dense box-local map of d^2 at the
//                   target surface voxels, a negative sentinel elsewhere, +inf where the source surface is empty.
//   sd_summary      what the three metrics need from such a map, reduced on the device: the number of surface voxels, the
//                   counts with sqrt(d^2) <= tau_j, the sum of sqrt(d^2) over the finite entries, the number of infinite
//                   ones, and the order statistics of d^2 at up to 4 ranks.  Counts: integer atomics.  Sum: a fixed grid of
//                   SD_SUM_BLOCKS x 256 threads, a fixed tree per block, then a fixed tree over the block partials (same bits
//                   on every run and every device).  Order statistics: radix select, 8 bits a pass from the top, over the
//                   64-bit patterns of the non-negative doubles (they order like unsigned integers); all ranks share a pass.
//
// HBM / cache bound; nothing here is MFMA-shaped.
#include "common.h"
#include "hd_scan.h"

namespace {

constexpr double SD_SENTINEL = -1.0;
constexpr int SD_MAX_TOL = 8, SD_MAX_RANK = 4;
constexpr int SD_SUM_BLOCKS = 1024;
constexpr int SD_PASSES = 8;

// out record, 8 bytes a slot
constexpr int SD_OUT_N = 0, SD_OUT_INF = 1, SD_OUT_SUM = 2, SD_OUT_TOL = 3, SD_OUT_RANK = 11, SD_OUT_SLOTS = 16;

// scratch: histograms [pass][rank][256] u64 | block partial sums | select state (prefix, remaining rank)
constexpr size_t SD_HIST_BYTES = (size_t)SD_PASSES * SD_MAX_RANK * 256 * 8;
constexpr size_t SD_PART_BYTES = (size_t)SD_SUM_BLOCKS * 8;
constexpr size_t SD_STATE_BYTES = 256;
constexpr size_t SD_SCRATCH_BYTES = SD_HIST_BYTES + SD_PART_BYTES + SD_STATE_BYTES;

struct SdSpacing { double z, y, x; };
struct SdQuery {
    double tol[SD_MAX_TOL];
    unsigned long long rank[SD_MAX_RANK];
    int ntol, nrank;
};

MSSEG_DEVFN double sd_sq(double s, int k) {
#pragma clang fp contract(off)
    const double t = s * (double)k;
    return t * t;
}

// pass y: h[z][y][x] = min over y' of (sx gx[z][y'][x])^2 + (sy (y - y'))^2, searched outward from y until (sy k)^2 >= best
__global__ __launch_bounds__(256) void sd_pass_y_kernel(const unsigned short* __restrict__ gx, HdBox b, SdSpacing sp,
                                                        double* __restrict__ h) {
#pragma clang fp contract(off)
    const int by = b.y1 - b.y0, bx = b.x1 - b.x0, bz = b.z1 - b.z0;
    const long long V = (long long)bz * by * bx;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % bx), y = (int)((i / bx) % by);
        const long long base = i - (long long)y * bx;          // (z, 0, x)
        double best = __builtin_inf();
        const int kmax = y > by - 1 - y ? y : by - 1 - y;
        for (int k = 0; k <= kmax; ++k) {
            const double k2 = sd_sq(sp.y, k);
            if (k2 >= best) break;
            if (y - k >= 0) {
                const int g = gx[base + (long long)(y - k) * bx];
                if (g != HD_INF16) { const double v = sd_sq(sp.x, g) + k2; best = v < best ? v : best; }
            }
            if (k && y + k < by) {
                const int g = gx[base + (long long)(y + k) * bx];
                if (g != HD_INF16) { const double v = sd_sq(sp.x, g) + k2; best = v < best ? v : best; }
            }
        }
        h[i] = best;
    }
}

// pass z at the surface voxels of class `cls` in `tgt`; the sentinel everywhere else
__global__ __launch_bounds__(256) void sd_pass_z_kernel(const double* __restrict__ h, const unsigned char* __restrict__ tgt,
                                                        int cls, int H, int W, HdBox b, SdSpacing sp,
                                                        double* __restrict__ d2) {
#pragma clang fp contract(off)
    const int by = b.y1 - b.y0, bx = b.x1 - b.x0, bz = b.z1 - b.z0;
    const long long V = (long long)bz * by * bx, plane = (long long)by * bx;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < V; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % bx), y = (int)((i / bx) % by), z = (int)(i / plane);
        if (tgt[((long long)(b.z0 + z) * H + (b.y0 + y)) * W + b.x0 + x] != cls) { d2[i] = SD_SENTINEL; continue; }
        double best = __builtin_inf();
        const int kmax = z > bz - 1 - z ? z : bz - 1 - z;
        for (int k = 0; k <= kmax; ++k) {
            const double k2 = sd_sq(sp.z, k);
            if (k2 >= best) break;
            if (z - k >= 0) { const double v = h[i - (long long)k * plane] + k2; best = v < best ? v : best; }
            if (k && z + k < bz) { const double v = h[i + (long long)k * plane] + k2; best = v < best ? v : best; }
        }
        d2[i] = best;                                           // +inf: the source surface is empty
    }
}

// counts (integer atomics) and the block's partial of the sum of sqrt(d2); grid = SD_SUM_BLOCKS, whatever n is
__global__ __launch_bounds__(256) void sd_count_kernel(const double* __restrict__ d2, long long n, SdQuery q,
                                                       unsigned long long* __restrict__ out, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double ssum[256];
    __shared__ unsigned int scnt[2 + SD_MAX_TOL];
    if (threadIdx.x < 2 + SD_MAX_TOL) scnt[threadIdx.x] = 0;
    __syncthreads();
    double sum = 0.0;
    unsigned int cnt = 0, cinf = 0, ctol[SD_MAX_TOL] = {};
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)SD_SUM_BLOCKS * 256) {
        const double v = d2[i];
        if (!(v >= 0.0)) continue;
        ++cnt;
        const double d = sqrt(v);
        if (v == __builtin_inf()) ++cinf; else sum += d;
#pragma unroll
        for (int j = 0; j < SD_MAX_TOL; ++j) ctol[j] += (j < q.ntol && d <= q.tol[j]) ? 1u : 0u;
    }
    if (cnt) {
        atomicAdd(&scnt[0], cnt);
        if (cinf) atomicAdd(&scnt[1], cinf);
#pragma unroll
        for (int j = 0; j < SD_MAX_TOL; ++j) if (ctol[j]) atomicAdd(&scnt[2 + j], ctol[j]);
    }
    ssum[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) ssum[threadIdx.x] += ssum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = ssum[0];
    if (threadIdx.x < 2 + SD_MAX_TOL && scnt[threadIdx.x]) {
        const int slot = threadIdx.x == 0 ? SD_OUT_N : (threadIdx.x == 1 ? SD_OUT_INF : SD_OUT_TOL + (int)threadIdx.x - 2);
        atomicAdd(out + slot, (unsigned long long)scnt[threadIdx.x]);
    }
}

__global__ void sd_select_init_kernel(SdQuery q, unsigned long long* __restrict__ state) {
    const int r = threadIdx.x;
    if (r < SD_MAX_RANK) { state[r] = 0ull; state[SD_MAX_RANK + r] = r < q.nrank ? q.rank[r] : 0ull; }
}

// one radix pass: per rank, the histogram of byte (7 - pass) over the entries whose higher bytes equal the rank's prefix
__global__ __launch_bounds__(256) void sd_select_hist_kernel(const double* __restrict__ d2, long long n, int pass, int nrank,
                                                             const unsigned long long* __restrict__ state,
                                                             unsigned long long* __restrict__ hist /* [rank][256] */) {
    __shared__ unsigned int lh[SD_MAX_RANK][256];
    for (int r = 0; r < SD_MAX_RANK; ++r) lh[r][threadIdx.x] = 0;
    __syncthreads();
    unsigned long long prefix[SD_MAX_RANK];
#pragma unroll
    for (int r = 0; r < SD_MAX_RANK; ++r) prefix[r] = state[r];
    const int shift = 56 - 8 * pass;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = d2[i];
        if (!(v >= 0.0)) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
        const unsigned long long high = pass ? bits >> (shift + 8) : 0ull;
        const int digit = (int)((bits >> shift) & 255ull);
#pragma unroll
        for (int r = 0; r < SD_MAX_RANK; ++r)
            if (r < nrank && high == prefix[r]) atomicAdd(&lh[r][digit], 1u);
    }
    __syncthreads();
    for (int r = 0; r < nrank; ++r)
        if (lh[r][threadIdx.x]) atomicAdd(hist + r * 256 + threadIdx.x, (unsigned long long)lh[r][threadIdx.x]);
}

// the digit that holds each rank's remaining position; a rank past the last entry runs into byte 0xFF on every pass and
// ends as the all-ones pattern (a NaN)
__global__ void sd_select_step_kernel(const unsigned long long* __restrict__ hist, int nrank,
                                      unsigned long long* __restrict__ state) {
    const int r = threadIdx.x;
    if (r >= nrank) return;
    unsigned long long k = state[SD_MAX_RANK + r], cum = 0;
    int d = -1;
    for (int j = 0; j < 256; ++j) {
        const unsigned long long c = hist[r * 256 + j];
        if (cum + c > k) { d = j; break; }
        cum += c;
    }
    if (d < 0) { d = 255; cum = 0; }                             // past the last entry: the remaining rank stays
    state[r] = (state[r] << 8) | (unsigned long long)d;
    state[SD_MAX_RANK + r] = k - cum;
}

__global__ __launch_bounds__(256) void sd_finish_kernel(const double* __restrict__ part, int nrank,
                                                        const unsigned long long* __restrict__ state,
                                                        unsigned long long* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double ssum[256];
    double s = 0.0;
    for (int j = 0; j < SD_SUM_BLOCKS / 256; ++j) s += part[threadIdx.x * (SD_SUM_BLOCKS / 256) + j];
    ssum[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) ssum[threadIdx.x] += ssum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[SD_OUT_SUM] = (unsigned long long)__double_as_longlong(ssum[0]);
    if ((int)threadIdx.x < nrank) out[SD_OUT_RANK + threadIdx.x] = state[threadIdx.x];
}

}  // namespace

extern "C" {

size_t msseg_sd_directed_workspace_bytes(int bz, int by, int bx) {
    const size_t v = (size_t)bz * by * bx;
    return ((v * 2 + 255) / 256) * 256 + v * 8;
}

int msseg_sd_directed_mm(const uint8_t* edges_src, const uint8_t* edges_tgt, int cls, int D, int H, int W, const int* box6,
                         const double* spacing3, void* workspace, size_t workspace_bytes, double* d2map,
                         msseg_stream_t stream) {
    if (!edges_src || !edges_tgt || !box6 || !spacing3 || cls < 0 || cls > 254)
        MSSEG_FAIL(MSSEG_EINVAL, "sd_directed_mm: bad args");
    for (int a = 0; a < 3; ++a)
        if (!(spacing3[a] > 0.0) || !(spacing3[a] < __builtin_inf()))
            MSSEG_FAIL(MSSEG_EINVAL, "sd_directed_mm: spacing (%g, %g, %g) must be finite and positive", spacing3[0],
                       spacing3[1], spacing3[2]);
    HdBox b{box6[0], box6[1], box6[2], box6[3], box6[4], box6[5]};
    if (b.z0 < 0 || b.y0 < 0 || b.x0 < 0 || b.z1 > D || b.y1 > H || b.x1 > W || b.z0 >= b.z1 || b.y0 >= b.y1 || b.x0 >= b.x1)
        MSSEG_FAIL(MSSEG_EINVAL, "sd_directed_mm: box [%d,%d)x[%d,%d)x[%d,%d) outside %dx%dx%d", b.z0, b.z1, b.y0, b.y1, b.x0,
                   b.x1, D, H, W);
    const int bz = b.z1 - b.z0, by = b.y1 - b.y0, bx = b.x1 - b.x0;
    if (bx >= HD_INF16) MSSEG_FAIL(MSSEG_EINVAL, "sd_directed_mm: box too wide");
    if (!workspace || !d2map) MSSEG_FAIL(MSSEG_EINVAL, "sd_directed_mm: no workspace or no output map");
    if (workspace_bytes < msseg_sd_directed_workspace_bytes(bz, by, bx))
        MSSEG_FAIL(MSSEG_EWORKSPACE, "sd_directed_mm: workspace %zu B < %zu B", workspace_bytes,
                   msseg_sd_directed_workspace_bytes(bz, by, bx));
    const size_t v = (size_t)bz * by * bx;
    unsigned short* gx = (unsigned short*)workspace;
    double* h = (double*)((char*)workspace + ((v * 2 + 255) / 256) * 256);
    const SdSpacing sp{spacing3[0], spacing3[1], spacing3[2]};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(hd_pass_x_kernel, dim3(stream_grid((long long)bz * by, 64)), dim3(256), 0, s, edges_src, cls, H, W, b, gx);
    hipLaunchKernelGGL(sd_pass_y_kernel, dim3(stream_grid((long long)v)), dim3(256), 0, s, gx, b, sp, h);
    hipLaunchKernelGGL(sd_pass_z_kernel, dim3(stream_grid((long long)v)), dim3(256), 0, s, h, edges_tgt, cls, H, W, b, sp, d2map);
    MSSEG_CHECK_LAUNCH("sd_directed_mm");
    return MSSEG_OK;
}

size_t msseg_sd_summary_scratch_bytes(void) { return SD_SCRATCH_BYTES; }

int msseg_sd_summary(const double* d2map, long long n, const double* tolerances, int ntol, const long long* ranks, int nrank,
                     void* scratch, size_t scratch_bytes, void* out16, msseg_stream_t stream) {
    if (!d2map || !scratch || !out16 || n < 1 || ntol < 0 || ntol > SD_MAX_TOL || nrank < 0 || nrank > SD_MAX_RANK ||
        (ntol && !tolerances) || (nrank && !ranks))
        MSSEG_FAIL(MSSEG_EINVAL, "sd_summary: bad args (%lld entries, %d tolerances of at most %d, %d ranks of at most %d)", n,
                   ntol, SD_MAX_TOL, nrank, SD_MAX_RANK);
    if (((uintptr_t)scratch & 7) || ((uintptr_t)out16 & 7) || scratch_bytes < SD_SCRATCH_BYTES)
        MSSEG_FAIL(MSSEG_EWORKSPACE, "sd_summary: needs an 8-byte aligned scratch of %zu bytes (got %zu)", SD_SCRATCH_BYTES,
                   scratch_bytes);
    SdQuery q{};
    q.ntol = ntol;
    q.nrank = nrank;
    for (int j = 0; j < ntol; ++j) {
        if (tolerances[j] != tolerances[j]) MSSEG_FAIL(MSSEG_EINVAL, "sd_summary: tolerance %d is NaN", j);
        q.tol[j] = tolerances[j];
    }
    for (int r = 0; r < nrank; ++r) {
        if (ranks[r] < 0) MSSEG_FAIL(MSSEG_EINVAL, "sd_summary: rank %d is negative", r);
        q.rank[r] = (unsigned long long)ranks[r];
    }
    unsigned long long* hist = (unsigned long long*)scratch;
    double* part = (double*)((char*)scratch + SD_HIST_BYTES);
    unsigned long long* state = (unsigned long long*)((char*)scratch + SD_HIST_BYTES + SD_PART_BYTES);
    unsigned long long* out = (unsigned long long*)out16;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, SD_HIST_BYTES, s) != hipSuccess || hipMemsetAsync(out, 0, SD_OUT_SLOTS * 8, s) != hipSuccess)
        MSSEG_FAIL(MSSEG_ELAUNCH, "sd_summary: memset failed");
    hipLaunchKernelGGL(sd_select_init_kernel, dim3(1), dim3(64), 0, s, q, state);
    hipLaunchKernelGGL(sd_count_kernel, dim3(SD_SUM_BLOCKS), dim3(256), 0, s, d2map, n, q, out, part);
    if (nrank)
        for (int p = 0; p < SD_PASSES; ++p) {
            unsigned long long* hp = hist + (size_t)p * SD_MAX_RANK * 256;
            hipLaunchKernelGGL(sd_select_hist_kernel, dim3(stream_grid(n)), dim3(256), 0, s, d2map, n, p, nrank, state, hp);
            hipLaunchKernelGGL(sd_select_step_kernel, dim3(1), dim3(64), 0, s, hp, nrank, state);
        }
    hipLaunchKernelGGL(sd_finish_kernel, dim3(1), dim3(256), 0, s, part, nrank, state, out);
    MSSEG_CHECK_LAUNCH("sd_summary");
    return MSSEG_OK;
}

}  // extern "C"
