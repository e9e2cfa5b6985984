// Intensity half of the nnU-Net augmentation recipe on a gathered batch: Gaussian noise, Gaussian
// blur, contrast, gamma on the inverted image, gamma -- in that order, per (patch, channel) row of a device table.
//
//   front_kernel       x -> w: optional noise (Philox4x32-10 keyed by the row, counter = voxel index, Box-Muller) fused into
//                      the tile load of the optional separable blur (scipy gaussian_filter, mode reflect, truncate 4); a
//                      halo voxel reads the noise of its SOURCE voxel, so a reflected tap sees the mirrored voxel's noise.
//                      Epilogue: per-block partials {sum, sum of squares, min, max} of what it wrote.
//   stage_kernel<0>    contrast:  clip((x - m) f + m, lo, hi), statistics from the previous writer's partials; epilogue
//                      partials of its own output.
//   stage_kernel<1>    gamma, reduction only: sum and sum of squares of y = ((v - lo) / (R + 1e-7))^g R + lo.
//   stage_kernel<2>    gamma, apply: recomputes y and retains the statistics, (y - mean y) / (std y + 1e-8) s + m; epilogue
//                      partials again.  The inverted pass runs the same two kernels on v = -x and negates back.
//
// Every reduction is per-thread accumulation in double, a fixed wave-shuffle tree, a fixed-order sum over the waves and a
// partial per block; the consumer combines the partials of its row in a fixed order, in double.  No floating-point atomics:
// two calls with the same input and table give the same bits.  The working buffer is the fp32 output itself, or the
// workspace when the output is bf16; the last launched kernel converts.
#include <cmath>

#include "common.h"

namespace {

typedef msseg_intensity_row Row;

constexpr int TZ = 8, TY = 8;          // output tile of the front kernel: 8 x 8 x TX, TX = 32 (radius <= 4) or 16 (radius <= 8)
constexpr int NT = 256;                 // contrast / gamma kernels
constexpr int NTF = 512;                // front kernel: its LDS tile allows two blocks per CU, so the waves come from the block

// ---- Philox4x32-10 (Salmon et al., SC'11): counter = {voxel index lo, hi, 0, 0}, key = the row's 64 bits ----------------
MSSEG_DEVFN void philox4x32_10(unsigned long long ctr, unsigned long long key, uint32_t w[4]) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0u, c3 = 0u;
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// standard normal of (key, voxel index): words 0 and 1 -> uniforms ((bits >> 8) + 0.5) 2^-24 in (0, 1], Box-Muller cosine
// branch; cospif(2 u) keeps the argument reduction exact
MSSEG_DEVFN float normal_of(unsigned long long key, long long i) {
    uint32_t w[4];
    philox4x32_10((unsigned long long)i, key, w);
    const float u1 = ((float)(w[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float u2 = ((float)(w[1] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// scipy mode "reflect": d c b a | a b c d | d c b a; one reflection is enough for radius <= 8 <= n
MSSEG_DEVFN int reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

MSSEG_DEVFN void store_val(void* dst, int dst_bf16, long long i, float v) {
    if (dst_bf16) ((bf16_t*)dst)[i] = (bf16_t)v;
    else ((float*)dst)[i] = v;
}

// ---- block-wide {sum, sumsq, min, max} in a fixed order; the result is broadcast to every thread ---------------------------
struct Stat4 { double s, ss, mn, mx; };

template <int NTn = NT>
MSSEG_DEVFN Stat4 block_reduce4(Stat4 v, double* red /* [NTn / 64][4] in LDS */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v.s += __shfl_xor(v.s, o);
        v.ss += __shfl_xor(v.ss, o);
        v.mn = fmin(v.mn, __shfl_xor(v.mn, o));
        v.mx = fmax(v.mx, __shfl_xor(v.mx, o));
    }
    __syncthreads();                                           // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) {
        double* r = red + (threadIdx.x >> 6) * 4;
        r[0] = v.s; r[1] = v.ss; r[2] = v.mn; r[3] = v.mx;
    }
    __syncthreads();
    Stat4 t = {red[0], red[1], red[2], red[3]};
#pragma unroll
    for (int w = 1; w < NTn / 64; ++w) {
        t.s += red[w * 4]; t.ss += red[w * 4 + 1];
        t.mn = fmin(t.mn, red[w * 4 + 2]); t.mx = fmax(t.mx, red[w * 4 + 3]);
    }
    return t;
}

// the n partials of one row -> its statistics (thread t takes partials t, t + NT, ... in order, then the tree above)
MSSEG_DEVFN Stat4 combine_partials(const double* __restrict__ part, int n, double* red) {
    Stat4 v = {0.0, 0.0, INFINITY, -INFINITY};
    for (int j = threadIdx.x; j < n; j += NT) {
        const double* p = part + (long long)j * 4;
        v.s += p[0]; v.ss += p[1]; v.mn = fmin(v.mn, p[2]); v.mx = fmax(v.mx, p[3]);
    }
    return block_reduce4(v, red);
}

MSSEG_DEVFN void acc(Stat4& a, float v) {
    const double d = (double)v;
    a.s += d; a.ss += d * d; a.mn = fmin(a.mn, d); a.mx = fmax(a.mx, d);
}

// 2 R + 1 symmetric taps around p, `stride` apart: the loads first, then w0 c + sum_k w_k (a_-k + a_+k) in the order k = 1 .. R
template <int R> MSSEG_DEVFN float taps(const float* p, int stride, const float* w) {
    float v[2 * R + 1];
#pragma unroll
    for (int k = -R; k <= R; ++k) v[k + R] = p[k * stride];
    float s = w[0] * v[R];
#pragma unroll
    for (int k = 1; k <= R; ++k) s = fmaf(w[k], v[R - k] + v[R + k], s);
    return s;
}
// the radius is uniform over the block: a scalar branch to the unrolled body
MSSEG_DEVFN float taps_of(int r, const float* p, int stride, const float* w) {
    switch (r) {
        case 1: return taps<1>(p, stride, w);
        case 2: return taps<2>(p, stride, w);
        case 3: return taps<3>(p, stride, w);
        case 4: return taps<4>(p, stride, w);
        case 5: return taps<5>(p, stride, w);
        case 6: return taps<6>(p, stride, w);
        case 7: return taps<7>(p, stride, w);
        default: return taps<8>(p, stride, w);
    }
}

// ---- front: copy / noise / blur -------------------------------------------------------------------------------------------
// grid (tiles, N * C); dynamic LDS: A[(8 + 2 rc)^2 (TX + 2 rc)] + B[(8 + 2 rc)^2 TX] floats, rc = the batch's largest radius
template <int TX>
__global__ __launch_bounds__(NTF) void front_kernel(const float* __restrict__ x, const Row* __restrict__ rows, void* dst,
                                                   int dst_bf16, int D, int H, int W, int tiles_y, int tiles_x, int rcap,
                                                   double* __restrict__ stats) {
    extern __shared__ float lds[];
    __shared__ float wts[9];
    __shared__ double red[NTF / 64 * 4];
    const int tid = threadIdx.x, pc = blockIdx.y;
    const Row row = rows[pc];
    const bool noise = (row.mask & MSSEG_INTENSITY_NOISE) != 0;
    int r = (row.mask & MSSEG_INTENSITY_BLUR) ? (int)(4.0f * row.blur_sigma + 0.5f) : 0;
    r = r > rcap ? rcap : r;                                   // the host has refused larger radii; never index past the LDS
    const bool blur = r > 0;                                   // radius 0 is the single tap of weight 1
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, tz = blockIdx.x / (tiles_x * tiles_y);
    const int z0 = tz * TZ, y0 = ty * TY, x0 = tx * TX;
    const int ez = min(TZ, D - z0), ey = min(TY, H - y0), ex = min(TX, W - x0);
    const int az = ez + 2 * r, ay = ey + 2 * r, ax = ex + 2 * r;
    const long long V = (long long)D * H * W, base = (long long)pc * V;
    const float sigma_n = row.noise_std;
    const unsigned long long key = row.noise_key;
    Stat4 st = {0.0, 0.0, INFINITY, -INFINITY};

    if (blur && tid <= r) {                                    // exp(-k^2 / (2 sigma^2)) normalised over the 2 r + 1 taps
        const double s2 = (double)row.blur_sigma * (double)row.blur_sigma;
        double sum = 1.0;
        for (int k = 1; k <= r; ++k) sum += 2.0 * exp(-0.5 * k * k / s2);
        wts[tid] = (float)(exp(-0.5 * tid * tid / s2) / sum);
    }

    float* A = lds;
    float* B = lds + (TZ + 2 * rcap) * (TY + 2 * rcap) * (TX + 2 * rcap);
    // tile (+ halo) load; without blur r == 0, the tile is the output and goes straight out
    const unsigned total = (unsigned)(az * ay * ax);
#pragma unroll 4                                               // four independent loads in flight per thread
    for (unsigned idx = tid; idx < total; idx += NTF) {
        const unsigned lx = idx % (unsigned)ax, t = idx / (unsigned)ax, ly = t % (unsigned)ay, lz = t / (unsigned)ay;
        const int gz = reflect(z0 - r + (int)lz, D), gy = reflect(y0 - r + (int)ly, H), gx = reflect(x0 - r + (int)lx, W);
        const long long i = ((long long)gz * H + gy) * W + gx;
        float v = x[base + i];
        if (noise) v += sigma_n * normal_of(key, i);
        if (blur) A[idx] = v;
        else {
            store_val(dst, dst_bf16, base + i, v);
            acc(st, v);
        }
    }
    if (blur) {
        __syncthreads();
        // along x: A[az][ay][ax] -> B[az][ay][TX]
        const int rows_a = az * ay;
        for (int idx = tid; idx < rows_a * TX; idx += NTF) {
            const int ox = idx & (TX - 1), rw = idx / TX;
            if (ox >= ex) continue;
            B[idx] = taps_of(r, A + rw * ax + ox + r, 1, wts);
        }
        __syncthreads();
        // along y: B[az][ay][TX] -> C[az][TY][TX] (in A's place)
        float* Cb = A;
        for (int idx = tid; idx < az * TY * TX; idx += NTF) {
            const int ox = idx & (TX - 1), oy = (idx / TX) & (TY - 1), lz = idx / (TX * TY);
            if (ox >= ex || oy >= ey) continue;
            Cb[idx] = taps_of(r, B + (lz * ay + oy + r) * TX + ox, TX, wts);
        }
        __syncthreads();
        // along z: C -> global
        for (int idx = tid; idx < TZ * TY * TX; idx += NTF) {
            const int ox = idx & (TX - 1), oy = (idx / TX) & (TY - 1), oz = idx / (TX * TY);
            if (ox >= ex || oy >= ey || oz >= ez) continue;
            const float s = taps_of(r, Cb + ((oz + r) * TY + oy) * TX + ox, TY * TX, wts);
            store_val(dst, dst_bf16, base + ((long long)(z0 + oz) * H + (y0 + oy)) * W + (x0 + ox), s);
            acc(st, s);
        }
    }
    if (stats) {
        const Stat4 t = block_reduce4<NTF>(st, red);
        if (tid == 0) {
            double* p = stats + ((long long)pc * gridDim.x + blockIdx.x) * 4;
            p[0] = t.s; p[1] = t.ss; p[2] = t.mn; p[3] = t.mx;
        }
    }
}

// ---- contrast / gamma -----------------------------------------------------------------------------------------------------
struct StageArgs {
    const Row* rows;
    float* w;            // working batch (fp32), updated in place
    void* out;           // != NULL: this is the last launch; it writes `out` (for every row, converting when out_bf16)
    int out_bf16;
    unsigned bit;        // the stage's mask bit
    int invert;          // gamma on the inverted image
    long long V;
    const double* s0; int n0;      // partials written by the front kernel / contrast / gamma-inverted apply, and how many
    const double* s1; const double* s2; int ne;
    double* s_out;       // this launch's partials of its own output (apply kernels), or NULL
    double* q;           // gamma: {sum y, sum y^2} partials, [N * C][ne][4] (two used)
};

MSSEG_DEVFN float gamma_curve(float v, float lo, float R, float g) {
    return powf((v - lo) / (R + 1e-7f), g) * R + lo;
}

// MODE 0: contrast apply; 1: gamma reduce; 2: gamma apply.  grid (ne, N * C)
template <int MODE>
__global__ __launch_bounds__(NT) void stage_kernel(StageArgs a) {
    __shared__ double red[NT / 64 * 4];
    const int tid = threadIdx.x, pc = blockIdx.y;
    const Row row = a.rows[pc];
    const long long base = (long long)pc * a.V;
    const long long step = (long long)gridDim.x * NT, first = (long long)blockIdx.x * NT + tid;
    const float* src = a.w + base;                             // may alias dst: every thread rewrites what it read
    const bool final_ = a.out != nullptr;
    if (!(row.mask & a.bit)) {
        // not chosen: nothing to do, except that the last launch still owes the row to a separate output
        if (MODE != 1 && final_ && a.out != (void*)a.w)
            for (long long i = first; i < a.V; i += step) store_val(a.out, a.out_bf16, base + i, src[i]);
        return;
    }
    // the statistics of the row as it stands: the partials of the last kernel that wrote it
    const double* part; int np;
    if (a.bit == MSSEG_INTENSITY_CONTRAST || !(row.mask & (MSSEG_INTENSITY_CONTRAST | MSSEG_INTENSITY_GAMMA_INV)) ||
        (a.bit == MSSEG_INTENSITY_GAMMA_INV && !(row.mask & MSSEG_INTENSITY_CONTRAST))) {
        part = a.s0 + (long long)pc * a.n0 * 4; np = a.n0;
    } else if (a.bit == MSSEG_INTENSITY_GAMMA && (row.mask & MSSEG_INTENSITY_GAMMA_INV)) {
        part = a.s2 + (long long)pc * a.ne * 4; np = a.ne;
    } else {
        part = a.s1 + (long long)pc * a.ne * 4; np = a.ne;
    }
    const Stat4 in = combine_partials(part, np, red);
    const double n = (double)a.V, mean = in.s / n;
    const double var = fmax(in.ss / n - mean * mean, 0.0);
    void* dst = final_ ? a.out : (void*)a.w;
    const int dst_bf16 = final_ ? a.out_bf16 : 0;
    Stat4 st = {0.0, 0.0, INFINITY, -INFINITY};

    if (MODE == 0) {
        const float m = (float)mean, lo = (float)in.mn, hi = (float)in.mx, f = row.contrast;
#pragma unroll 4
        for (long long i = first; i < a.V; i += step) {
            const float v = fminf(fmaxf((src[i] - m) * f + m, lo), hi);
            store_val(dst, dst_bf16, base + i, v);
            acc(st, v);
        }
    } else {
        const float sgn = a.invert ? -1.0f : 1.0f;
        const float lo = a.invert ? -(float)in.mx : (float)in.mn;
        const float R = (float)in.mx - (float)in.mn;
        const float g = a.invert ? row.gamma_inv : row.gamma;
        if (MODE == 1) {
#pragma unroll 4
            for (long long i = first; i < a.V; i += step) {
                const double y = (double)gamma_curve(sgn * src[i], lo, R, g);
                st.s += y; st.ss += y * y;
            }
            const Stat4 t = block_reduce4(st, red);
            if (tid == 0) {
                double* p = a.q + ((long long)pc * a.ne + blockIdx.x) * 4;
                p[0] = t.s; p[1] = t.ss; p[2] = 0.0; p[3] = 0.0;
            }
            return;
        }
        const Stat4 qy = combine_partials(a.q + (long long)pc * a.ne * 4, a.ne, red);
        const double my = qy.s / n, sy = sqrt(fmax(qy.ss / n - my * my, 0.0));
        const float myf = (float)my, scale = (float)(sqrt(var) / (sy + 1e-8)), mv = sgn * (float)mean;
#pragma unroll 4
        for (long long i = first; i < a.V; i += step) {
            const float y = gamma_curve(sgn * src[i], lo, R, g);
            const float v = sgn * ((y - myf) * scale + mv);
            store_val(dst, dst_bf16, base + i, v);
            acc(st, v);
        }
    }
    if (a.s_out) {
        const Stat4 t = block_reduce4(st, red);
        if (tid == 0) {
            double* p = a.s_out + ((long long)pc * a.ne + blockIdx.x) * 4;
            p[0] = t.s; p[1] = t.ss; p[2] = t.mn; p[3] = t.mx;
        }
    }
}

__global__ __launch_bounds__(NT) void noise_bits_kernel(unsigned long long key, long long first, long long n, uint32_t* out) {
    const long long j = (long long)blockIdx.x * NT + threadIdx.x;
    if (j >= n) return;
    uint32_t w[4];
    philox4x32_10((unsigned long long)(first + j), key, w);
    for (int k = 0; k < 4; ++k) out[j * 4 + k] = w[k];
}

// ---- host side ------------------------------------------------------------------------------------------------------------
int tiles_of(int D, int H, int W, int tx) { return ceil_div(D, TZ) * ceil_div(H, TY) * ceil_div(W, tx); }
int stage_blocks(long long V) {
    const long long b = ceil_div_ll(V, 4 * NT);
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}
size_t front_lds_bytes(int tx, int rc) {
    return (size_t)(TZ + 2 * rc) * (TY + 2 * rc) * (2 * tx + 2 * rc) * sizeof(float);
}

struct Plan { size_t s0, s1, s2, q, w, total; int nf_max, ne; };
bool plan_of(int N, int C, int D, int H, int W, Plan* p) {
    if (N < 1 || C < 1 || (long long)N * C > 65535 || D < 8 || H < 8 || W < 8 || D > 4096 || H > 4096 || W > 4096) return false;
    const long long NC = (long long)N * C, V = (long long)D * H * W;
    p->nf_max = tiles_of(D, H, W, 16);
    p->ne = stage_blocks(V);
    size_t o = 0;
    p->s0 = o; o += (size_t)NC * p->nf_max * 4 * sizeof(double);
    p->s1 = o; o += (size_t)NC * p->ne * 4 * sizeof(double);
    p->s2 = o; o += (size_t)NC * p->ne * 4 * sizeof(double);
    p->q = o;  o += (size_t)NC * p->ne * 4 * sizeof(double);
    p->w = o;  o += (size_t)NC * V * sizeof(float);
    p->total = o;
    return true;
}

}  // namespace

extern "C" {

size_t msseg_intensity_aug_workspace_bytes(int N, int C, int D, int H, int W) {
    Plan p;
    return plan_of(N, C, D, H, W, &p) ? p.total : 0;
}

int msseg_intensity_aug(const float* x, const msseg_intensity_row* rows_host, const void* rows_dev, int N, int C, int D, int H,
                        int W, void* out, int out_dtype, void* workspace, size_t workspace_bytes, msseg_stream_t stream) {
    if (!x || !rows_host || !rows_dev || !out || (const void*)x == out) MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: bad pointers");
    if (out_dtype != MSSEG_F32 && out_dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: bad dtype");
    Plan p;
    if (!plan_of(N, C, D, H, W, &p))
        MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: %d x %d rows of %d x %d x %d: every patch dimension must be in 8..4096 and "
                   "N * C <= 65535", N, C, D, H, W);
    const int NC = N * C;
    unsigned any = 0;
    int rmax = 0;
    for (int j = 0; j < NC; ++j) {
        const msseg_intensity_row& r = rows_host[j];
        if (r.mask & ~0x1fu) MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: row %d: unknown stage bits 0x%x", j, r.mask);
        if ((r.mask & MSSEG_INTENSITY_NOISE) && !(r.noise_std >= 0.0f && std::isfinite(r.noise_std)))
            MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: row %d: noise std %g", j, (double)r.noise_std);
        if (r.mask & MSSEG_INTENSITY_BLUR) {
            if (!(r.blur_sigma > 0.0f && r.blur_sigma <= 2.0f))
                MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: row %d: blur sigma %g is outside (0, 2] (radius <= 8)", j,
                           (double)r.blur_sigma);
            const int rad = (int)(4.0f * r.blur_sigma + 0.5f);
            rmax = rad > rmax ? rad : rmax;
        }
        if ((r.mask & MSSEG_INTENSITY_CONTRAST) && !std::isfinite(r.contrast))
            MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: row %d: contrast factor %g", j, (double)r.contrast);
        if ((r.mask & MSSEG_INTENSITY_GAMMA_INV) && !(r.gamma_inv > 0.0f && std::isfinite(r.gamma_inv)))
            MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: row %d: gamma (inverted) %g", j, (double)r.gamma_inv);
        if ((r.mask & MSSEG_INTENSITY_GAMMA) && !(r.gamma > 0.0f && std::isfinite(r.gamma)))
            MSSEG_FAIL(MSSEG_EINVAL, "intensity_aug: row %d: gamma %g", j, (double)r.gamma);
        any |= r.mask;
    }
    const unsigned later = any & (MSSEG_INTENSITY_CONTRAST | MSSEG_INTENSITY_GAMMA_INV | MSSEG_INTENSITY_GAMMA);
    if (later && (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < p.total))
        MSSEG_FAIL(MSSEG_EWORKSPACE, "intensity_aug: needs a 16-byte aligned workspace of %zu bytes", p.total);
    hipStream_t s = (hipStream_t)stream;
    const Row* rows = (const Row*)rows_dev;
    const int out_bf16 = out_dtype == MSSEG_BF16;
    char* ws = (char*)workspace;
    // the working batch: the fp32 output itself, or the workspace when the output is bf16
    float* wbuf = !later ? nullptr : (out_bf16 ? (float*)(ws + p.w) : (float*)out);
    double* s0 = later ? (double*)(ws + p.s0) : nullptr;

    const int tx = rmax > 4 ? 16 : 32;
    const int nf = tiles_of(D, H, W, tx);
    const size_t lds = rmax > 0 ? front_lds_bytes(tx, rmax) : 0;
    void* fdst = later ? (void*)wbuf : out;
    const int fbf16 = later ? 0 : out_bf16;
    dim3 fgrid((unsigned)nf, (unsigned)NC);
    if (tx == 32) {
        static msseg_lds_attr_once once;
        if (!once.ensure((const void*)front_kernel<32>, (int)front_lds_bytes(32, 4)))
            MSSEG_FAIL(MSSEG_ELAUNCH, "intensity_aug: cannot reserve %zu bytes of LDS", front_lds_bytes(32, 4));
        hipLaunchKernelGGL(front_kernel<32>, fgrid, dim3(NTF), lds, s, x, rows, fdst, fbf16, D, H, W, ceil_div(H, TY),
                           ceil_div(W, 32), rmax, s0);
    } else {
        static msseg_lds_attr_once once;
        if (!once.ensure((const void*)front_kernel<16>, (int)front_lds_bytes(16, 8)))
            MSSEG_FAIL(MSSEG_ELAUNCH, "intensity_aug: cannot reserve %zu bytes of LDS", front_lds_bytes(16, 8));
        hipLaunchKernelGGL(front_kernel<16>, fgrid, dim3(NTF), lds, s, x, rows, fdst, fbf16, D, H, W, ceil_div(H, TY),
                           ceil_div(W, 16), rmax, s0);
    }
    MSSEG_CHECK_LAUNCH("intensity_aug (noise / blur)");
    if (!later) return MSSEG_OK;

    StageArgs a;
    a.rows = rows; a.w = wbuf; a.out_bf16 = out_bf16; a.V = (long long)D * H * W;
    a.s0 = s0; a.n0 = nf; a.s1 = (double*)(ws + p.s1); a.s2 = (double*)(ws + p.s2); a.ne = p.ne; a.q = (double*)(ws + p.q);
    dim3 grid((unsigned)p.ne, (unsigned)NC);
    const unsigned last = (later & MSSEG_INTENSITY_GAMMA) ? MSSEG_INTENSITY_GAMMA
                        : (later & MSSEG_INTENSITY_GAMMA_INV) ? MSSEG_INTENSITY_GAMMA_INV : MSSEG_INTENSITY_CONTRAST;
    if (later & MSSEG_INTENSITY_CONTRAST) {
        a.bit = MSSEG_INTENSITY_CONTRAST; a.invert = 0;
        a.out = last == a.bit ? out : nullptr; a.s_out = last == a.bit ? nullptr : (double*)(ws + p.s1);
        hipLaunchKernelGGL(stage_kernel<0>, grid, dim3(NT), 0, s, a);
        MSSEG_CHECK_LAUNCH("intensity_aug (contrast)");
    }
    for (int inv = 1; inv >= 0; --inv) {
        const unsigned bit = inv ? MSSEG_INTENSITY_GAMMA_INV : MSSEG_INTENSITY_GAMMA;
        if (!(later & bit)) continue;
        a.bit = bit; a.invert = inv;
        a.out = nullptr; a.s_out = nullptr;
        hipLaunchKernelGGL(stage_kernel<1>, grid, dim3(NT), 0, s, a);
        MSSEG_CHECK_LAUNCH("intensity_aug (gamma statistics)");
        a.out = last == bit ? out : nullptr; a.s_out = last == bit ? nullptr : (double*)(ws + p.s2);
        hipLaunchKernelGGL(stage_kernel<2>, grid, dim3(NT), 0, s, a);
        MSSEG_CHECK_LAUNCH("intensity_aug (gamma)");
    }
    return MSSEG_OK;
}

int msseg_intensity_noise_bits(unsigned key_lo, unsigned key_hi, long long first, long long n, uint32_t* out,
                               msseg_stream_t stream) {
    const unsigned long long key = (unsigned long long)key_hi << 32 | key_lo;
    if (!out || n < 1 || first < 0) MSSEG_FAIL(MSSEG_EINVAL, "intensity_noise_bits: bad args");
    hipLaunchKernelGGL(noise_bits_kernel, dim3((unsigned)ceil_div_ll(n, NT)), dim3(NT), 0, (hipStream_t)stream, key, first, n, out);
    MSSEG_CHECK_LAUNCH("intensity_noise_bits");
    return MSSEG_OK;
}

}  // extern "C"
