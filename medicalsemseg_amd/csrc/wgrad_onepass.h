// One-pass weight gradient (bf16) for gfx950: dW[m][k] = sum_t P[t][m] * Q[t][k] over many "tokens" t, where Q[t] is row t of x
// and P[t] is the row of dy that a compile-time ROW SOURCE assigns to token t (linear_wgrad.hip describes the scheme and its
// measurements).  A workgroup reads whole token rows (its slice of the output: NTP x NTQ 16-wide tiles), keeps its partial dW
// in registers across all its 128-token chunks and writes ONE partial block; the callers add the blocks in a fixed order.
//
// Per chunk: 256 threads load the rows (16-byte pieces, consecutive lanes on consecutive pieces of a row) into registers while
// the previous chunk is computed, then store them as [32-channel block][token][96 B] images (64 B of data, 32 B pad: the pitch
// that makes the transposing reads conflict-free, as in igemm_wgrad.hip); wave w takes tokens 32 w .. 32 w + 31 as its MFMA
// k-step: both operands are read with ds_read_b64_tr_b16 (contraction index = token, memory holds token rows), NTP + NTQ
// fragments for NTP x NTQ (+ NTP with bias sums) MFMAs.
#pragma once
#include "common.h"

constexpr int LWG_TT = 128;            // tokens per chunk
constexpr int LWG_RS = 96;             // LDS row pitch of a 32-channel block image
constexpr int LWG_BLK_BYTES = LWG_TT * LWG_RS;
constexpr int LWG_THREADS = 256;

struct LwgParams {
    const void* x; long long ldx;      // [NV][K]
    const void* dy; long long lddy;    // what the row source reads
    float* part;                       // [slice][workgroup][ [k: NTQ*16][m: NTP*16] (+ bias [NTP*16]) ] fp32
    long long NV;
    int nchunks;
    int kslices;                       // RowsPlain / RowsDeconvK2: blockIdx.y = ms * kslices + ks
    int D, H, W, cout;                 // RowsDeconvK2 / RowsDeconvK4: coarse grid; RowsDeconvK2: channels of the fine tensor
};

// ---- row sources: what differs between the users of the kernel ------------------------------------------------------
//   BIAS    the column sums of P are accumulated too (one more MFMA per row tile against ones) and follow the block
//   TABLE   table entries per chunk (LWG_TT or 0): entry(p, n, d, h, w) of a token's coarse voxel, filled by the first 128 threads
//   slice   decodes blockIdx.y; qoff = byte offset of the slice in a row of x
//   chunk   what the pieces of the chunk that starts at token t0 are addressed from
//   piece   address of 16-byte piece c of row `row` of the chunk with base pb = chunk(p, t0) and table tab

// dy [NV][M] as it lies in memory (Linear layers): slice (ms, ks)
template <int NTP, int NTQ> struct RowsPlain {
    static constexpr bool BIAS = true;
    static constexpr int TABLE = 0;
    static constexpr const char* NAME = "lwg_kernel";
    const unsigned char* pg;
    int qoff;
    bool with_bias;
    MSSEG_DEVFN RowsPlain(const LwgParams& p, unsigned y) {
        const int ms = y / p.kslices, ks = y - ms * p.kslices;
        pg = (const unsigned char*)p.dy + (long long)ms * NTP * 32;
        qoff = ks * NTQ * 32;
        with_bias = ks == 0;
    }
    MSSEG_DEVFN const unsigned char* chunk(const LwgParams& p, long long t0) const { return pg + t0 * p.lddy * 2; }
    MSSEG_DEVFN const unsigned char* piece(const LwgParams& p, const unsigned char* pb, const unsigned* tab, int row, int c) const {
        return pb + (unsigned)(row * (int)p.lddy * 2 + c * 16);
    }
};

// dy = the FINE tensor [N, 2D, 2H, 2W, cout] of a ConvTranspose3d k2 s2: the row of coarse token t is its 8 child rows
// (m = abc * cout + co), gathered while staging; slice (ms, ks) of M = 8 * cout.  Fine voxel count < 2^31.
template <int NTP, int NTQ> struct RowsDeconvK2 {
    static constexpr bool BIAS = false;
    static constexpr int TABLE = LWG_TT;
    static constexpr const char* NAME = "lwg_kernel<deconv>";
    int ms, qoff;
    MSSEG_DEVFN RowsDeconvK2(const LwgParams& p, unsigned y) {
        ms = y / p.kslices;
        qoff = (y - ms * p.kslices) * NTQ * 32;
    }
    // fine voxel (2d, 2h, 2w)
    MSSEG_DEVFN unsigned entry(const LwgParams& p, unsigned n, unsigned d, unsigned h, unsigned w) const {
        return ((n * 2u * p.D + 2u * d) * 2u * p.H + 2u * h) * 2u * p.W + 2u * w;
    }
    // piece c of the slice = channels (ms * NTP * 2 + c) * 8 .. of the gathered row: child abc, channel co
    MSSEG_DEVFN const unsigned char* chunk(const LwgParams& p, long long t0) const { return (const unsigned char*)p.dy; }
    MSSEG_DEVFN const unsigned char* piece(const LwgParams& p, const unsigned char* pb, const unsigned* tab, int row, int c) const {
        const unsigned ch = (unsigned)(ms * NTP * 2 + c) * 8u;
        const unsigned abc = ch / (unsigned)p.cout, co = ch - abc * (unsigned)p.cout;
        const unsigned fv = tab[row < LWG_TT ? row : 0] + ((abc >> 2) * 2u * p.H + ((abc >> 1) & 1u)) * 2u * p.W + (abc & 1u);
        return pb + ((unsigned long long)fv * (unsigned)p.lddy + co) * 2;
    }
};

// dy = the FINE tensor [N, 4D, 4H, 4W, COUT] of a ConvTranspose3d k4 s4.  For a fixed fine row ab the children c of a coarse
// voxel are adjacent fine voxels: slice (ab, child group cg) with CH adjacent child rows (CH * COUT channels).
template <int CH, int COUT> struct RowsDeconvK4 {
    static constexpr bool BIAS = false;
    static constexpr int TABLE = LWG_TT;
    static constexpr const char* NAME = "dc4_wgrad_kernel";
    static constexpr int NCG = 4 / CH, qoff = 0;
    int ab, cg;
    MSSEG_DEVFN RowsDeconvK4(const LwgParams& p, unsigned y) {
        ab = y / NCG;
        cg = y - ab * NCG;
    }
    // fine voxel (4d + a, 4h + b, 4w + cg * CH)
    MSSEG_DEVFN unsigned entry(const LwgParams& p, unsigned n, unsigned d, unsigned h, unsigned w) const {
        return ((n * 4u * p.D + 4u * d + (unsigned)(ab >> 2)) * 4u * p.H + 4u * h + (unsigned)(ab & 3)) * 4u * p.W + 4u * w +
               (unsigned)(cg * CH);
    }
    MSSEG_DEVFN const unsigned char* chunk(const LwgParams& p, long long t0) const { return (const unsigned char*)p.dy; }
    MSSEG_DEVFN const unsigned char* piece(const LwgParams& p, const unsigned char* pb, const unsigned* tab, int row, int c) const {
        const unsigned ch = (unsigned)c * 8u;
        const unsigned cl = ch / (unsigned)COUT, co = ch - cl * (unsigned)COUT;
        const unsigned fv = tab[row < LWG_TT ? row : 0] + cl;
        return pb + ((unsigned long long)fv * (unsigned long long)p.lddy + co) * 2;
    }
};

// floats of a workgroup's partial block
template <int NTP, int NTQ, class SRC> constexpr int lwg_part_floats() { return NTP * 16 * NTQ * 16 + (SRC::BIAS ? NTP * 16 : 0); }

template <int NTP, int NTQ, class SRC>
__global__ __launch_bounds__(LWG_THREADS, 1) void lwg_kernel(const LwgParams p) {
    constexpr int TT = LWG_TT, RS = LWG_RS, BLK_BYTES = LWG_BLK_BYTES;
    constexpr int NBP = (NTP + 1) / 2, NBQ = (NTQ + 1) / 2;       // 32-channel block images
    constexpr int CHP = NTP * 2, CHQ = NTQ * 2;                   // 16-byte pieces per row of the slice
    constexpr int NLP = (TT * CHP + LWG_THREADS - 1) / LWG_THREADS; // staged pieces per thread
    constexpr int NLQ = (TT * CHQ + LWG_THREADS - 1) / LWG_THREADS;
    constexpr int PART = lwg_part_floats<NTP, NTQ, SRC>();
    extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
    unsigned char* ldsP = smem;
    unsigned char* ldsQ = smem + NBP * BLK_BYTES;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const SRC src(p, blockIdx.y);
    const unsigned char* qg = (const unsigned char*)p.x + src.qoff;

    // ---- staging: piece i of the chunk = (row i / CH, 16-byte piece i % CH of the slice's part of the row); the offsets are
    // recomputed per chunk (constant divisions) instead of held in 3 registers per piece: the accumulators need the room
    u32x4_t sp[NLP], sq[NLQ];
    __shared__ unsigned fbase[2][SRC::TABLE ? SRC::TABLE : 1];
    auto fill_table = [&](int chunk, int sel) {
        if constexpr (SRC::TABLE != 0) {
            if (tid < TT) {
                unsigned t = (unsigned)chunk * (unsigned)TT + (unsigned)tid;
                if ((long long)t >= p.NV) t = 0;
                const unsigned w = t % (unsigned)p.W; t /= (unsigned)p.W;
                const unsigned h = t % (unsigned)p.H; t /= (unsigned)p.H;
                const unsigned d = t % (unsigned)p.D, n = t / (unsigned)p.D;
                fbase[sel][tid] = src.entry(p, n, d, h, w);
            }
        }
    };
    auto fetch = [&](int chunk, int tsel) {
        const long long t0 = (long long)chunk * TT;
        const int rows = (p.NV - t0) < TT ? (int)(p.NV - t0) : TT;
        const unsigned char* pb = src.chunk(p, t0);
        const unsigned char* qb = qg + t0 * p.ldx * 2;
#pragma unroll
        for (int it = 0; it < NLP; ++it) {
            const int i = tid + it * LWG_THREADS, row = i / CHP, c = i - row * CHP;
            sp[it] = row < rows ? *(const u32x4_t*)src.piece(p, pb, fbase[tsel], row, c) : u32x4_t{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int it = 0; it < NLQ; ++it) {
            const int i = tid + it * LWG_THREADS, row = i / CHQ, c = i - row * CHQ;
            sq[it] = row < rows ? *(const u32x4_t*)(qb + (unsigned)(row * (int)p.ldx * 2 + c * 16)) : u32x4_t{0u, 0u, 0u, 0u};
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int it = 0; it < NLP; ++it) {
            const int i = tid + it * LWG_THREADS, row = i / CHP, c = i - row * CHP;
            if (row < TT) *(u32x4_t*)(ldsP + (c >> 2) * BLK_BYTES + row * RS + (c & 3) * 16) = sp[it];
        }
#pragma unroll
        for (int it = 0; it < NLQ; ++it) {
            const int i = tid + it * LWG_THREADS, row = i / CHQ, c = i - row * CHQ;
            if (row < TT) *(u32x4_t*)(ldsQ + (c >> 2) * BLK_BYTES + row * RS + (c & 3) * 16) = sq[it];
        }
    };

    // ---- transposing fragment reads: lane = 16 g + 4 qr + pc supplies row 8 g + 4 i + qr of the wave's 32 tokens, channels
    // 4 pc .. of a 16-channel tile (cdna_hip_programming.md T10)
    const int g = lane >> 4, qr = (lane >> 2) & 3, pc = lane & 3;
    int trow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) trow[i] = (wave * 32 + 8 * g + 4 * i + qr) * RS + pc * 8;

    f32x4_t acc[NTP][NTQ], accb[SRC::BIAS ? NTP : 1];
#pragma unroll
    for (int a = 0; a < NTP; ++a) {
        if constexpr (SRC::BIAS) accb[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < NTQ; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const u32x4_t ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};   // bf16 1.0 x 8

    if constexpr (SRC::TABLE != 0) {
        fill_table(blockIdx.x, 0);
        __syncthreads();
    }
    if ((int)blockIdx.x < p.nchunks) fetch(blockIdx.x, 0);
    int tsel = 0;
    for (int chunk = blockIdx.x; chunk < p.nchunks; chunk += gridDim.x) {
        __syncthreads();                 // the previous chunk's fragment reads are done
        commit();
        tsel ^= 1;
        fill_table(chunk + gridDim.x, tsel);   // read by the fetch behind the next barrier; the other half is still the table of
                                               // the pieces in flight ... which were fetched before this point
        __syncthreads();
        if (chunk + (int)gridDim.x < p.nchunks) fetch(chunk + gridDim.x, tsel);
        u32x4_t pf[NTP], qf[NTQ];
#pragma unroll
        for (int a = 0; a < NTP; ++a) pf[a] = tr_frag(ldsP + (a >> 1) * BLK_BYTES, trow[0] + (a & 1) * 32, trow[1] + (a & 1) * 32);
#pragma unroll
        for (int b = 0; b < NTQ; ++b) qf[b] = tr_frag(ldsQ + (b >> 1) * BLK_BYTES, trow[0] + (b & 1) * 32, trow[1] + (b & 1) * 32);
#pragma unroll
        for (int a = 0; a < NTP; ++a) {
#pragma unroll
            for (int b = 0; b < NTQ; ++b) mma_chunk<bf16_t>(acc[a][b], pf[a], qf[b]);
            if constexpr (SRC::BIAS)
                if (src.with_bias) mma_chunk<bf16_t>(accb[a], pf[a], ones);
        }
    }

    // ---- the four waves' partial sums (different tokens) meet in LDS, [wave][k][m] so that a lane's four consecutive m are one
    // 16-byte store, and are added in a fixed order: ONE block [k][m] (+ the bias sums) per workgroup goes to memory
    __syncthreads();                     // the images are dead
    float* xch = (float*)smem;
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int a = 0; a < NTP; ++a) {
#pragma unroll
        for (int b = 0; b < NTQ; ++b)
            *(f32x4_t*)(xch + wave * PART + (b * 16 + r) * (NTP * 16) + a * 16 + q * 4) = acc[a][b];
        if constexpr (SRC::BIAS)
            if (r == 0) *(f32x4_t*)(xch + wave * PART + NTQ * 16 * NTP * 16 + a * 16 + q * 4) = accb[a];
    }
    __syncthreads();
    float* out = p.part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * PART;
    for (int i = tid * 4; i < PART; i += LWG_THREADS * 4) {
        const f32x4_t v0 = *(const f32x4_t*)(xch + i), v1 = *(const f32x4_t*)(xch + PART + i),
                      v2 = *(const f32x4_t*)(xch + 2 * PART + i), v3 = *(const f32x4_t*)(xch + 3 * PART + i);
        *(f32x4_t*)(out + i) = (v0 + v1) + (v2 + v3);
    }
}

// workgroups per slice: the chip divided by the slices, at least two chunks each when there are that many tokens (every
// workgroup writes a partial block whatever it summed), bounded by the partial blocks the workspace holds (fit, per slice)
static inline int lwg_grid_x(int slices, int nchunks, size_t fit) {
    int gx = msseg_num_cus() / slices;
    if (gx > (nchunks + 1) / 2) gx = (nchunks + 1) / 2;
    if ((size_t)gx > fit) gx = (int)fit;
    return gx < 1 ? 1 : gx;
}

// launches lwg_kernel<NTP, NTQ, SRC> on gx workgroups for each of `slices` slices; who: the caller, for error messages
template <int NTP, int NTQ, class SRC> int lwg_launch(const LwgParams& p, int gx, int slices, const char* who, hipStream_t stream) {
    constexpr int NBP = (NTP + 1) / 2, NBQ = (NTQ + 1) / 2;
    constexpr int PART = lwg_part_floats<NTP, NTQ, SRC>();
    constexpr int lds = (NBP + NBQ) * LWG_BLK_BYTES > 4 * PART * 4 ? (NBP + NBQ) * LWG_BLK_BYTES : 4 * PART * 4;
    static_assert(lds + 2 * SRC::TABLE * 4 <= 160 * 1024, "LDS budget");
    // the staging offsets inside a chunk are 32-bit
    if ((long long)LWG_TT * (p.ldx > p.lddy ? p.ldx : p.lddy) * 2 >= 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "%s: row stride too large", who);
    auto kern = lwg_kernel<NTP, NTQ, SRC>;
    static msseg_lds_attr_once attr;
    if (!attr.ensure((const void*)kern, lds)) MSSEG_FAIL(MSSEG_ELAUNCH, "%s: cannot set dynamic LDS size %d", who, lds);
    MSSEG_KTIMED(SRC::NAME, stream, hipLaunchKernelGGL(kern, dim3(gx, slices), dim3(LWG_THREADS), lds, stream, p));
    MSSEG_CHECK_LAUNCH(who);
    return MSSEG_OK;
}
