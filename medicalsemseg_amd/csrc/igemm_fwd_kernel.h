// Implicit-GEMM forward-shaped convolutions on MFMA (gfx950).
//
//   D[cout][voxel] = sum_{tap, c} W[cout][tap][c] * X[voxel + tap][c]
//
// One persistent workgroup walks output tiles.  Per tile and per block of CB = 4 chunks of input
// channels (32 bf16 / 16 f32) it stages
//   A: the input halo tile, channel-chunk-planar  [quarter q][halo voxel][16 B]
//   B: the packed weights for that channel block  [tap][q][cout][16 B]   (resident across tiles when
//      the layer has a single channel block)
// in LDS, then every wave runs NTAPS x MT x NT MFMA k-groups with both operands read as ds_read_b128.
// The planar A image keeps the 16 voxel rows of an MFMA operand on 16 consecutive 16-byte slots for
// every tap shift, and plane strides are multiples of 256 B, so the reads are bank-conflict free.
// Weights are the MFMA "A" operand (rows = cout) so that each lane ends up with 4 consecutive output
// channels of one voxel and the epilogue stores 8 B (bf16) / 16 B (f32) per lane.
//
// Source modes (how the A tile is filled) and epilogues cover: conv k3 s1 p1 (+ its input gradient with
// flipped weights), conv k1, few-channel convs gathered im2col-style (stem conv, patch embedding),
// ConvTranspose k2 s2 forward (1x1 GEMM + pixel-shuffle scatter) and its input gradient (gather).
//
// This header only defines the templates.  Every instantiation of the kernel lives in exactly one igemm_*.hip file, behind
// one of the msseg_igemm_* launchers of k3pp.h; igemm_fwd.hip (plans, validation, C entry points) instantiates none.
#pragma once
#include "common.h"
#include "k3pp.h"

#include <stdlib.h>
#include <type_traits>

// outside the anonymous namespace: the msseg_igemm_* launchers pass it between translation units
struct IgemmParams {
    const void* x;
    long long ldx;
    const void* wp;
    const float* bias;
    void* y;
    long long ldy;
    int N, D, H, W;      // tiled output grid (flat mode: N = D = H = 1, W = number of output voxels)
    int ID, IH, IW;      // source spatial dims (gather / deconv modes)
    int OD, OH, OW;      // output spatial dims of one sample (flat modes that need coordinates)
    int K, M, NKB;       // logical input channels, logical output channels, channel blocks
    int tiles_d, tiles_h, tiles_w;
    int ntiles;
    int cin, k, s, p;    // gather: real Cin, kernel, stride, pad
    int creal;           // deconv modes: real channel count of the fine tensor
    int vec_store;       // y / ldy allow 4-element vector stores
    int rel32_ok;        // halo-relative element offsets fit 32 bits (precomputed-offset staging path)
    int cout_block;      // 0 = msseg_cout_block(M)
    K3Fused fused;       // optional fused reductions of the stored output (k3pp.h)
    int* resident_out;   // host side only: non-null asks launch_cfg for the resident workgroups per CU instead of a launch
};

namespace {

enum { SRC_DIRECT = 0, SRC_GATHER = 1, SRC_DECONV_BWD = 2 };
enum { EPI_STORE = 0, EPI_DECONV = 1 };

template <typename T, int NTAPS, int SRC, int EPI, int TD, int TH, int TW, int WAVES, int NT, int STRIDE = 1>
struct IgemmCfg {
    static constexpr int EPC = DT<T>::EPC;
    static constexpr int CB = 4 * EPC;
    static constexpr int PAD = (NTAPS == 27) ? 1 : 0;
    // input halo of an output tile: (T-1)*STRIDE + kernel extent
    static constexpr int PD = (TD - 1) * STRIDE + 1 + 2 * PAD, PH = (TH - 1) * STRIDE + 1 + 2 * PAD,
                         PW = (TW - 1) * STRIDE + 1 + 2 * PAD;
    static constexpr int HV = PD * PH * PW;
    static constexpr int TV = TD * TH * TW;
    static constexpr int MT = TV / 16 / WAVES;
    static constexpr int NTHREADS = WAVES * 64;
    static constexpr int COUTB = NT * 16;
    static constexpr int PLANE = ((HV * 16 + 255) / 256) * 256;
    static constexpr int A_BYTES = ((4 * PLANE + 64 + 255) / 256) * 256;
    static constexpr int B_BYTES = NTAPS * 4 * COUTB * 16;
    // Statistics area (EPI_STORE): the per-wave staging of a flush [WAVES][COUTB][2] first, because its size is fixed, then one
    // (sum, sum of squares) slot [COUTB][2] per sample of the launch.  The launch passes lds_bytes(samples of the launch), so a
    // training batch does not pay LDS for MSSEG_STATS_NMAX samples: on the 4x4x8 tile with 32-wide cout blocks that is the
    // difference between one and two resident workgroups per CU (80 640 B at N = 2 against 82 432 B).  Nothing reads or
    // writes past the last slot, so there is no pad behind it; LEGACY_LDS_BYTES is the size every launch passed before
    // (NMAX slots + a 256 B pad), kept for the one-workgroup-per-CU switch of launch_cfg and as the registered maximum.
    static constexpr int WPART_FLOATS = (EPI == EPI_STORE) ? WAVES * COUTB * 2 : 0;
    static constexpr int SLOT_FLOATS = (EPI == EPI_STORE) ? COUTB * 2 : 0;
    static constexpr int lds_bytes(int nslots) { return A_BYTES + B_BYTES + (WPART_FLOATS + nslots * SLOT_FLOATS) * 4; }
    static constexpr int LEGACY_LDS_BYTES = lds_bytes(MSSEG_STATS_NMAX) + ((EPI == EPI_STORE) ? 256 : 0);
    static_assert(TV % (16 * WAVES) == 0, "tile must split into 16-voxel MFMA tiles per wave");
};

MSSEG_DEVFN int aoff(int q, int plane) { return q * plane + (q >> 1) * 32; }

template <typename T, int NTAPS, int SRC, int EPI, int TD, int TH, int TW, int WAVES, int NT, int STRIDE = 1>
__global__ __launch_bounds__(WAVES * 64, 1) void igemm_fwd_kernel(const IgemmParams p) {
    using C = IgemmCfg<T, NTAPS, SRC, EPI, TD, TH, TW, WAVES, NT, STRIDE>;
    constexpr int EPC = C::EPC, CB = C::CB, PAD = C::PAD, PH = C::PH, PW = C::PW, HV = C::HV, MT = C::MT;
    constexpr int NTHREADS = C::NTHREADS, COUTB = C::COUTB, PLANE = C::PLANE;
    constexpr bool HREUSE = NTAPS == 27 && STRIDE == 1 && TW == 16 && TH % MT == 0;
    extern __shared__ __attribute__((aligned(256))) unsigned char smem[];
    unsigned char* ldsA = smem;
    unsigned char* ldsB = smem + C::A_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int coutblk = blockIdx.y;
    const T* __restrict__ xg = (const T*)p.x;
    T* __restrict__ yg = (T*)p.y;

    // per-lane LDS offsets of the voxel rows this lane feeds into the MFMA B operand
    int abase[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int v = (wave * MT + m) * 16 + r;
        const int td = v / (TH * TW), th = (v / TW) % TH, tw = v % TW;
        abase[m] = aoff(q, PLANE) + ((td * STRIDE * PH + th * STRIDE) * PW + tw * STRIDE) * 16;
    }
    const int bbase = (q * COUTB + r) * 16;
    float* wpart = (float*)(smem + C::A_BYTES + C::B_BYTES);  // [WAVES][COUTB][2] staging for the per-sample flush
    float* spart = wpart + C::WPART_FLOATS;                   // [p.N][COUTB][2] sample slots (IgemmCfg::lds_bytes)
    const bool do_stats = (EPI == EPI_STORE) && p.fused.stats != nullptr;
    if (do_stats) {
        for (int i = tid; i < p.N * C::SLOT_FLOATS; i += NTHREADS) spart[i] = 0.f;
    }
    float st[NT][4], st2[NT][4];  // this lane's running (sum, sum of squares) of the current sample
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) st[j][e] = st2[j][e] = 0.f;
    int cur_n = -1;
    // Flush = fixed-order reduction lanes -> wave -> workgroup, so the statistics are bit-reproducible.
    auto flush_stats = [&](int nn) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = st[j][e], b = st2[j][e];
#pragma unroll
                for (int o2 = 1; o2 < 16; o2 <<= 1) {
                    a += __shfl_xor(a, o2);
                    b += __shfl_xor(b, o2);
                }
                if (r == 0) {
                    const int cl = j * 16 + q * 4 + e;
                    wpart[(wave * COUTB + cl) * 2 + 0] = a;
                    wpart[(wave * COUTB + cl) * 2 + 1] = b;
                }
                st[j][e] = st2[j][e] = 0.f;
            }
        __syncthreads();
        if (tid < COUTB * 2) {
            float s = 0.f;
#pragma unroll
            for (int wv = 0; wv < WAVES; ++wv) s += wpart[wv * COUTB * 2 + tid];
            spart[nn * COUTB * 2 + tid] += s;
        }
        __syncthreads();
    };

    // ---------------------------------------------------------------------------------------------
    // Software pipeline over stages (tile, channel block): the global loads of stage s+1 are issued right
    // after stage s's LDS image is complete and stay in flight under stage s's MFMAs; they are written to
    // LDS after the barrier that ends stage s (issue-early / write-late register staging).
    // ---------------------------------------------------------------------------------------------
    constexpr int NIT_A = (HV * 4 + NTHREADS - 1) / NTHREADS;
    constexpr int NIT_B = (C::B_BYTES / 16 + NTHREADS - 1) / NTHREADS;
    struct TileCo { int n, d0, h0, w0; };
    auto decode = [&](int tile) {
        TileCo tc;
        int t = tile;
        tc.w0 = (t % p.tiles_w) * TW; t /= p.tiles_w;
        tc.h0 = (t % p.tiles_h) * TH; t /= p.tiles_h;
        tc.d0 = (t % p.tiles_d) * TD; t /= p.tiles_d;
        tc.n = t;
        return tc;
    };
    auto load_a_chunk = [&](const TileCo& tc, int kb, int i) -> u32x4_t {
        const int cq = i & 3, hv = i >> 2;
        const int c = kb * CB + cq * EPC;
        u32x4_t val = {0u, 0u, 0u, 0u};
        if constexpr (SRC == SRC_DIRECT) {
            const int hw = hv % PW, t2 = hv / PW, hh = t2 % PH, hd = t2 / PH;
            const int d = tc.d0 * STRIDE - PAD + hd, h = tc.h0 * STRIDE - PAD + hh, w = tc.w0 * STRIDE - PAD + hw;
            const int XD = STRIDE == 1 ? p.D : p.ID, XH = STRIDE == 1 ? p.H : p.IH, XW = STRIDE == 1 ? p.W : p.IW;
            if (c < p.K && (unsigned)d < (unsigned)XD && (unsigned)h < (unsigned)XH && (unsigned)w < (unsigned)XW) {
                const long long vox = (((long long)tc.n * XD + d) * XH + h) * XW + w;
                val = *(const u32x4_t*)(xg + vox * p.ldx + c);
            }
        } else if constexpr (SRC == SRC_GATHER) {
            const int ov = tc.w0 + hv;  // flat output voxel
            if (ov < p.W && c < p.K) {
                int tt = ov;
                const int ow = tt % p.OW; tt /= p.OW;
                const int oh = tt % p.OH; tt /= p.OH;
                const int od = tt % p.OD; const int nn = tt / p.OD;
                alignas(16) T tmp[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const int vc = c + e;
                    float fv = 0.f;
                    if (vc < p.K) {
                        const int tap = vc / p.cin, ci = vc - tap * p.cin;
                        const int kw = tap % p.k, kh = (tap / p.k) % p.k, kd = tap / (p.k * p.k);
                        const int id = od * p.s - p.p + kd, ih = oh * p.s - p.p + kh, iw = ow * p.s - p.p + kw;
                        if ((unsigned)id < (unsigned)p.ID && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW) {
                            const long long vox = (((long long)nn * p.ID + id) * p.IH + ih) * p.IW + iw;
                            fv = DT<T>::ld(xg + vox * p.ldx + ci);
                        }
                    }
                    DT<T>::st(&tmp[e], fv);
                }
                val = *(const u32x4_t*)tmp;
            }
        } else {  // SRC_DECONV_BWD: coarse voxel gathers its 8 fine children
            const int cv = tc.w0 + hv;
            if (cv < p.W && c < p.K) {
                int tt = tc.n * p.W + cv;   // flat index over all samples (p.N == 1: tc.n == 0)
                const int cw = tt % p.OW; tt /= p.OW;
                const int ch = tt % p.OH; tt /= p.OH;
                const int cd = tt % p.OD; const int nn = tt / p.OD;
                const int abc = c / p.creal, co = c - abc * p.creal;
                const int fd = 2 * cd + (abc >> 2), fh = 2 * ch + ((abc >> 1) & 1), fw = 2 * cw + (abc & 1);
                const long long vox = (((long long)nn * (2 * p.OD) + fd) * (2 * p.OH) + fh) * (2 * p.OW) + fw;
                val = *(const u32x4_t*)(xg + vox * p.ldx + co);
            }
        }
        return val;
    };
    u32x4_t pa[NIT_A], pb[NIT_B];
    // DIRECT source: the (halo voxel, chunk) a thread stages is the same for every tile, so its element offset
    // relative to the tile origin and its halo coordinates are computed once (VALU work per tile drops from ~40 to
    // ~3 instructions per chunk; interior tiles skip the bounds checks altogether).
    int a_rel[NIT_A];
    // small tiles also keep the packed halo coordinates (hd | hh << 8 | hw << 16): on the 24^3 ... 6^3 grids nearly every
    // tile is an edge tile and the bounds test runs inside the MFMA loop on one wave per SIMD, where recomputing the
    // coordinates (two divisions by constants per chunk) is exposed latency; the large tiles (NIT_A up to 17) recompute
    constexpr bool KEEP_PK = SRC == SRC_DIRECT && NIT_A <= 8;
    int a_pk[KEEP_PK ? NIT_A : 1];
    const int XD = STRIDE == 1 ? p.D : p.ID, XH = STRIDE == 1 ? p.H : p.IH, XW = STRIDE == 1 ? p.W : p.IW;
    if constexpr (SRC == SRC_DIRECT) {
#pragma unroll
        for (int it = 0; it < NIT_A; ++it) {
            const int i = tid + it * NTHREADS;
            const int cq = i & 3, hv = i >> 2;
            const int hw = hv % PW, t2 = hv / PW, hh = t2 % PH, hd = t2 / PH;
            a_rel[it] = (int)((((long long)hd * XH + hh) * XW + hw) * p.ldx) + cq * EPC;
            if constexpr (KEEP_PK) a_pk[it] = hd | (hh << 8) | (hw << 16);
        }
    }
    // The global loads of a stage are issued one at a time (fetch_a / fetch_b) from slots spread over the MFMA loop
    // of the previous stage, after fetch_setup() has fixed the stage's base pointers.
    const T* f_bp = xg;
    const u32x4_t* f_bsrc = nullptr;
    bool f_interior = false, f_cok = false;
    int f_dB = 0, f_hB = 0, f_wB = 0, f_kb = 0;
    TileCo f_tc{0, 0, 0, 0};
    auto fetch_setup = [&](const TileCo& tc, int kb) {
        f_tc = tc;
        f_kb = kb;
        if constexpr (SRC == SRC_DIRECT) {
            f_dB = tc.d0 * STRIDE - PAD; f_hB = tc.h0 * STRIDE - PAD; f_wB = tc.w0 * STRIDE - PAD;
            const long long basev = (((long long)tc.n * XD + f_dB) * XH + f_hB) * XW + f_wB;
            f_bp = xg + basev * p.ldx + kb * CB;
            f_interior = f_dB >= 0 && f_dB + C::PD <= XD && f_hB >= 0 && f_hB + PH <= XH && f_wB >= 0 && f_wB + PW <= XW;
            const int nchunk = (p.K - kb * CB + EPC - 1) / EPC;   // valid 16-byte chunks of this channel block
            f_cok = (tid & 3) < nchunk;
        }
        f_bsrc = (const u32x4_t*)((const unsigned char*)p.wp + ((long long)coutblk * p.NKB + kb) * C::B_BYTES);
    };
    auto fetch_a = [&](int it) {
        const int i = tid + it * NTHREADS;
        if constexpr (SRC == SRC_DIRECT) {
            if (p.rel32_ok) {
                bool ok = f_cok && i < HV * 4;
                if (!f_interior) {   // edge tile
                    int d, h, w;
                    if constexpr (KEEP_PK) {
                        const int pk = a_pk[it];
                        d = f_dB + (pk & 255); h = f_hB + ((pk >> 8) & 255); w = f_wB + (pk >> 16);
                    } else {         // recompute this chunk's halo coordinates (kept out of registers)
                        const int hv = i >> 2;
                        const int hw = hv % PW, t2 = hv / PW;
                        d = f_dB + t2 / PH; h = f_hB + t2 % PH; w = f_wB + hw;
                    }
                    ok = ok && (unsigned)d < (unsigned)XD && (unsigned)h < (unsigned)XH && (unsigned)w < (unsigned)XW;
                }
                pa[it] = ok ? *(const u32x4_t*)(f_bp + a_rel[it]) : u32x4_t{0u, 0u, 0u, 0u};
                return;
            }
        }
        pa[it] = (i < HV * 4) ? load_a_chunk(f_tc, f_kb, i) : u32x4_t{0u, 0u, 0u, 0u};
    };
    auto fetch_b = [&](int it) {
        const int i = tid + it * NTHREADS;
        pb[it] = (i < C::B_BYTES / 16) ? f_bsrc[i] : u32x4_t{0u, 0u, 0u, 0u};
    };
    auto fetch = [&](const TileCo& tc, int kb) {   // whole stage at once (prologue)
        fetch_setup(tc, kb);
#pragma unroll
        for (int it = 0; it < NIT_A; ++it) fetch_a(it);
#pragma unroll
        for (int it = 0; it < NIT_B; ++it) fetch_b(it);
    };
    auto commit = [&](bool with_b) {
#pragma unroll
        for (int it = 0; it < NIT_A; ++it) {
            const int i = tid + it * NTHREADS;
            if (i < HV * 4) *(u32x4_t*)(ldsA + aoff(i & 3, PLANE) + (i >> 2) * 16) = pa[it];
        }
        if (with_b) {
#pragma unroll
            for (int it = 0; it < NIT_B; ++it) {
                const int i = tid + it * NTHREADS;
                if (i < C::B_BYTES / 16) ((u32x4_t*)ldsB)[i] = pb[it];
            }
        }
    };

    f32x4_t acc[MT][NT];
    // Deferred epilogue stores: a finished tile's outputs are kept packed in registers and written at the START of
    // the next stage, BEFORE that stage's prefetch loads are issued.  The wait in front of the LDS commit
    // (s_waitcnt vmcnt(0) at the loop head) then only sees operations that had a whole MFMA phase to complete,
    // instead of stalling every tile on the write latency of stores issued just before it.
    using PendT = typename std::conditional<sizeof(T) == 2, bf16x4_t, f32x4_t>::type;
    PendT pend[MT][NT];
    TileCo ptc{0, 0, 0, 0};
    bool pend_valid = false;
    auto store_one = [&](int m, int j) {
        const int v = (wave * MT + m) * 16 + r;
        const int td = v / (TH * TW), th = (v / TW) % TH, tw = v % TW;
        const int d = ptc.d0 + td, h = ptc.h0 + th, w = ptc.w0 + tw;
        if (d >= p.D || h >= p.H || w >= p.W) return;
        const int co = coutblk * COUTB + j * 16 + q * 4;
        if (co + 4 > p.M) return;
        T* dst;
        if constexpr (EPI == EPI_STORE) {
            const long long vox = (((long long)ptc.n * p.D + d) * p.H + h) * p.W + w;
            dst = yg + vox * p.ldy + co;
        } else {
            int tt = w;
            const int dw = tt % p.OW; tt /= p.OW;
            const int dh = tt % p.OH; tt /= p.OH;
            const int dd = tt % p.OD, dn = tt / p.OD;
            const int abc = co / p.creal;
            const int cbase = co - abc * p.creal;
            const int fd = 2 * dd + (abc >> 2), fh = 2 * dh + ((abc >> 1) & 1), fw = 2 * dw + (abc & 1);
            const long long fv = (((long long)dn * (2 * p.OD) + fd) * (2 * p.OH) + fh) * (2 * p.OW) + fw;
            dst = yg + fv * p.ldy + cbase;
        }
        *(PendT*)dst = pend[m][j];
    };
    auto store_pending = [&]() {
        if (!pend_valid) return;
        pend_valid = false;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < NT; ++j) store_one(m, j);
    };
    int tile = blockIdx.x, kb = 0;
    TileCo tc = decode(tile < p.ntiles ? tile : 0);
    bool b_pending = true;   // the weight image stays resident across tiles when the layer has a single channel block
    if (tile < p.ntiles) fetch(tc, 0);
    while (tile < p.ntiles) {
        __syncthreads();  // everyone finished reading the previous stage's LDS image
        commit(b_pending);
        __syncthreads();
        // next stage: (tile, kb) advance kb fastest
        int ntile = tile, nkb = kb + 1;
        if (nkb == p.NKB) { nkb = 0; ntile = tile + gridDim.x; }
        const TileCo ntc = decode(ntile < p.ntiles ? ntile : 0);
        b_pending = p.NKB > 1;
        // Side work of this stage, issued from slots spread over the MFMA loop so that it overlaps the matrix pipe
        // instead of serialising all waves in front of it: the previous tile's output stores (held in pend[][]),
        // then the next stage's halo and weight loads.
        const bool st_now = pend_valid, ld_now = ntile < p.ntiles;
        pend_valid = false;
        fetch_setup(ntc, nkb);
        constexpr int NI_ST = MT * NT, NI = NI_ST + NIT_A + NIT_B;
        auto side_item = [&](int i) {
            if (i < NI_ST) {
                if (st_now) store_one(i / NT, i % NT);
            } else if (i < NI_ST + NIT_A) {
                if (ld_now) fetch_a(i - NI_ST);
            } else {
                if (ld_now && b_pending) fetch_b(i - NI_ST - NIT_A);
            }
        };

        const int n = tc.n, d0 = tc.d0, h0 = tc.h0, w0 = tc.w0;
        if (kb == 0) {
            if constexpr (EPI == EPI_STORE) {
                if (do_stats && n != cur_n) {
                    if (cur_n >= 0) flush_stats(cur_n);
                    cur_n = n;
                }
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[m][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        // ---------------- MFMA ----------------
        // Operand fragments are double-buffered in registers: the LDS reads of tap t+1 are issued before the
        // MFMAs of tap t, so the matrix pipe runs under one full LDS latency instead of waiting for it per pair.
        {
            u32x4_t af[2][MT], bf[2][NT];
            auto load_frags = [&](int t, int buf) {
                const int kd = t / 9, kh = (t / 3) % 3, kw = t % 3;
                const int toff = (NTAPS == 27) ? ((kd * PH + kh) * PW + kw) * 16 : 0;
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    bf[buf][j] = *(const u32x4_t*)(ldsB + bbase + t * (4 * COUTB * 16) + j * 256);
#pragma unroll
                for (int m = 0; m < MT; ++m) af[buf][m] = *(const u32x4_t*)(ldsA + abase[m] + toff);
            };
            if constexpr (HREUSE) {
                // Row-reuse order (k3, 16-wide tiles whose MT voxel rows per wave are consecutive in h): for a fixed
                // (kd, kw) an activation row of the halo feeds up to three output rows (kh = 0..2), so it is read from
                // LDS once instead of three times and the weights of the three kh taps stay in registers while the
                // MT+2 halo rows stream past: 108 fragment reads per stage instead of 162 for the same 216 MFMAs.
                u32x4_t wf[3][NT], xf[2];
                const int xb = abase[0];
                auto ldw = [&](int g, int kh) {
                    const int tap = (g / 3) * 9 + kh * 3 + (g % 3);
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        wf[kh][j] = *(const u32x4_t*)(ldsB + bbase + tap * (4 * COUTB * 16) + j * 256);
                };
                auto ldx = [&](int g, int hr, int buf) {
                    xf[buf] = *(const u32x4_t*)(ldsA + xb + (((g / 3) * PH + hr) * PW + (g % 3)) * 16);
                };
                constexpr int NSTEP = 9 * (MT + 2);
                ldw(0, 0); ldw(0, 1); ldw(0, 2);
                ldx(0, 0, 0);
#pragma unroll
                for (int g = 0; g < 9; ++g) {
#pragma unroll
                    for (int hr = 0; hr < MT + 2; ++hr) {
                        const int step = g * (MT + 2) + hr, cur = step & 1;
                        if (hr + 1 < MT + 2) ldx(g, hr + 1, cur ^ 1);
                        else if (g + 1 < 9) ldx(g + 1, 0, cur ^ 1);
#pragma unroll
                        for (int i = 0; i < NI; ++i)
                            if (i * NSTEP / NI == step) side_item(i);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int kh = 0; kh < 3; ++kh) {
                            const int m = hr - kh;
                            if (m >= 0 && m < MT) {
#pragma unroll
                                for (int j = 0; j < NT; ++j) mma_chunk<T>(acc[m][j], wf[kh][j], xf[cur]);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        // a kh tap's weights are free once its last output row is issued: refill for the next (kd, kw)
                        if (g + 1 < 9) {
                            if (hr == MT - 1) ldw(g + 1, 0);
                            if (hr == MT) ldw(g + 1, 1);
                            if (hr == MT + 1) ldw(g + 1, 2);
                        }
                    }
                }
            } else {
                load_frags(0, 0);
#pragma unroll
                for (int t = 0; t < NTAPS; ++t) {
                    const int cur = t & 1;
                    if (t + 1 < NTAPS) load_frags(t + 1, cur ^ 1);
#pragma unroll
                    for (int i = 0; i < NI; ++i)
                        if (i * NTAPS / NI == t) side_item(i);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int j = 0; j < NT; ++j) mma_chunk<T>(acc[m][j], bf[cur][j], af[cur][m]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // the held outputs are written by now: give them a definite (dead) state so they free their registers
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < NT; ++j) pend[m][j] = PendT{};
        if (kb == p.NKB - 1) {
            // ---------------- epilogue ----------------
    #pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int v = (wave * MT + m) * 16 + r;
                const int td = v / (TH * TW), th = (v / TW) % TH, tw = v % TW;
                const int d = d0 + td, h = h0 + th, w = w0 + tw;
                if (d >= p.D || h >= p.H || w >= p.W) continue;
                long long vox;
                int dn = 0, dd = 0, dh = 0, dw = 0;
                if constexpr (EPI == EPI_STORE) {
                    vox = (((long long)n * p.D + d) * p.H + h) * p.W + w;
                } else {
                    int tt = w;
                    dw = tt % p.OW; tt /= p.OW;
                    dh = tt % p.OH; tt /= p.OH;
                    dd = tt % p.OD; dn = tt / p.OD;
                    vox = 0;
                }
    #pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int co = coutblk * COUTB + j * 16 + q * 4;
                    if (co >= p.M) continue;
                    f32x4_t o = acc[m][j];
                    T* dst;
                    int cbase;
                    if constexpr (EPI == EPI_STORE) {
                        cbase = co;
                        dst = yg + vox * p.ldy + co;
                    } else {
                        const int abc = co / p.creal;
                        cbase = co - abc * p.creal;
                        const int fd = 2 * dd + (abc >> 2), fh = 2 * dh + ((abc >> 1) & 1), fw = 2 * dw + (abc & 1);
                        const long long fv = (((long long)dn * (2 * p.OD) + fd) * (2 * p.OH) + fh) * (2 * p.OW) + fw;
                        dst = yg + fv * p.ldy + cbase;
                    }
                    if (p.vec_store && co + 4 <= p.M) {
                        if (p.bias) {
    #pragma unroll
                            for (int e = 0; e < 4; ++e) o[e] += p.bias[cbase + e];
                        }
                        if constexpr (sizeof(T) == 2) {
                            pend[m][j] = bf16x4_t{(bf16_t)o[0], (bf16_t)o[1], (bf16_t)o[2], (bf16_t)o[3]};
                        } else {
                            pend[m][j] = o;
                        }
                    } else {
                        for (int e = 0; e < 4 && co + e < p.M; ++e) {
                            o[e] += (p.bias ? p.bias[cbase + e] : 0.f);
                            DT<T>::st(dst + e, o[e]);
                        }
                    }
                    if constexpr (EPI == EPI_STORE) {
                        if (do_stats) {
                            if (p.fused.nb_y == nullptr) {
    #pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const float rv = (float)(T)o[e];  // statistics of the tensor as stored
                                    st[j][e] += rv;
                                    st2[j][e] += rv * rv;
                                }
                            } else if (co + 4 <= p.M) {
                                // dz = da * lrelu'(a);  accumulate (sum dz, sum dz * yraw); xhat is formed at the end:
                                // sum dz*xhat = rstd * (sum dz*yraw - mean * sum dz)
                                f32x4_t yv, av;
                                if constexpr (sizeof(T) == 2) {
                                    const bf16x4_t y4 = *(const bf16x4_t*)((const T*)p.fused.nb_y + vox * p.fused.nb_ldy + co);
                                    const bf16x4_t a4 = *(const bf16x4_t*)((const T*)p.fused.nb_a + vox * p.fused.nb_lda + co);
    #pragma unroll
                                    for (int e = 0; e < 4; ++e) { yv[e] = (float)y4[e]; av[e] = (float)a4[e]; }
                                } else {
                                    yv = *(const f32x4_t*)((const T*)p.fused.nb_y + vox * p.fused.nb_ldy + co);
                                    av = *(const f32x4_t*)((const T*)p.fused.nb_a + vox * p.fused.nb_lda + co);
                                }
    #pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const float da = (float)(T)o[e];
                                    const float dz = av[e] > 0.f ? da : da * p.fused.nb_slope;
                                    st[j][e] += dz;
                                    st2[j][e] += dz * yv[e];
                                }
                            }
                        }
                    }
                }
            }
        }
        if (kb == p.NKB - 1 && p.vec_store) { ptc = tc; pend_valid = true; }
        tile = ntile; kb = nkb; tc = ntc;
    }
    store_pending();
    if constexpr (EPI == EPI_STORE) {
        if (do_stats) {
            if (cur_n >= 0) flush_stats(cur_n);
            __syncthreads();
            const int PN = p.N * COUTB * 2;
            float* wsp = p.fused.stats_ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * PN;
            for (int i = tid; i < PN; i += NTHREADS) wsp[i] = spart[i];
        }
    }
}

template <typename T, int NTAPS, int SRC, int EPI, int TD, int TH, int TW, int WAVES, int NT, int STRIDE = 1>
int launch_cfg(IgemmParams& p, hipStream_t stream) {
    using C = IgemmCfg<T, NTAPS, SRC, EPI, TD, TH, TW, WAVES, NT, STRIDE>;
    p.tiles_d = ceil_div(p.D, TD);
    p.tiles_h = ceil_div(p.H, TH);
    p.tiles_w = ceil_div(p.W, TW);
    const long long nt = (long long)p.N * p.tiles_d * p.tiles_h * p.tiles_w;
    if (nt > 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "igemm: too many tiles");
    p.ntiles = (int)nt;
    p.NKB = ceil_div(p.K, C::CB);
    p.vec_store = ((((uintptr_t)p.y) % (4 * sizeof(T))) == 0 && (p.ldy % 4) == 0) ? 1 : 0;
    {
        const long long xh = STRIDE == 1 ? p.H : p.IH, xw = STRIDE == 1 ? p.W : p.IW;
        p.rel32_ok = ((long long)(C::PD + 1) * xh * xw * p.ldx < 0x7fffffffLL) ? 1 : 0;
    }
    auto kern = igemm_fwd_kernel<T, NTAPS, SRC, EPI, TD, TH, TW, WAVES, NT, STRIDE>;
    static msseg_lds_attr_once attr;
    if (!attr.ensure((const void*)kern, C::LEGACY_LDS_BYTES))
        MSSEG_FAIL(MSSEG_ELAUNCH, "igemm: cannot set dynamic LDS size %d", C::LEGACY_LDS_BYTES);
    // Sample slots of the statistics area: the launch's N (validated against MSSEG_STATS_NMAX wherever statistics are asked
    // for; a plain launch of a larger batch never touches the area).  MSSEG_K3_MID_ONE_PER_CU=1 makes the 4x4x8 tile pass what
    // every launch passed before the area was sized by N: the same code at one workgroup per CU, for A/B runs in one build.
    static const bool legacy_lds = NTAPS == 27 && STRIDE == 1 && TD * TH * TW == 128 && [] {
        const char* e = getenv("MSSEG_K3_MID_ONE_PER_CU");
        return e != nullptr && *e != 0 && *e != '0';
    }();
    const int nslots = legacy_lds ? MSSEG_STATS_NMAX + 1 : (p.N < MSSEG_STATS_NMAX ? p.N : MSSEG_STATS_NMAX);
    const int lds = legacy_lds ? C::LEGACY_LDS_BYTES : C::lds_bytes(nslots);
    // The LDS-only rule every grid was sized by.  The flat and stride-2 families and the 2x4x8 conv tile keep it: their
    // registers allow another count than it answers (two or three where it says four; three where it says two), so the grid
    // of a long launch differs from what is resident; the number of partial rows of the fused sums, and with it their
    // summation order, follows from that grid and stays what it was.
    int wg_per_cu = (lds > 80 * 1024) ? 1 : ((lds > 40 * 1024) ? 2 : 4);
    if constexpr (NTAPS == 27 && STRIDE == 1) {
        // conv k3 tiles (k3_plan): the workgroups of this instantiation a CU holds at that LDS size, asked of the runtime once
        // per (instantiation, size).  It knows the registers the compiler used and the LDS allocation granule.
        static std::atomic<int> resident[MSSEG_STATS_NMAX + 2];
        int res = resident[nslots].load(std::memory_order_relaxed);
        if (res == 0) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&res, (const void*)kern, C::NTHREADS, lds) != hipSuccess || res < 1)
                MSSEG_FAIL(MSSEG_ELAUNCH, "igemm: no occupancy with %d bytes of LDS", lds);
            resident[nslots].store(res, std::memory_order_relaxed);
        }
        if (p.resident_out != nullptr) {   // msseg_conv3d_k3_resident_per_cu: the plan only, nothing is launched
            *p.resident_out = res;
            return MSSEG_OK;
        }
        if (TD * TH * TW != 64) wg_per_cu = res;   // the 4x4x8 and 4x8x16 tiles size their grid by it
    } else {
        if (p.resident_out != nullptr) MSSEG_FAIL(MSSEG_EINVAL, "igemm: the residency query is for the conv k3 tiles");
    }
    const int ncb = ceil_div(p.M, C::COUTB);
    int gx = msseg_num_cus() * wg_per_cu;
    if (gx > p.ntiles) gx = p.ntiles;
    if (EPI == EPI_STORE && p.fused.stats != nullptr) {
        // one partial row of N x COUTB x 2 floats per workgroup: no more workgroups than the reduce scratch holds rows of
        // (a persistent workgroup walks tiles in steps of the grid, so a smaller grid is only slower)
        const size_t row_bytes = (size_t)ncb * p.N * C::COUTB * 2 * sizeof(float);
        const size_t fit = (msseg_reduce_scratch_bytes() - MSSEG_SCRATCH_HEADER_BYTES) / row_bytes;
        if (fit < 1) MSSEG_FAIL(MSSEG_EWORKSPACE, "igemm: one row of fused sums (%zu bytes) exceeds the reduce scratch", row_bytes);
        if ((size_t)gx > fit) gx = (int)fit;
    }
    if (gx < 1) gx = 1;
    dim3 grid(gx, ncb, 1);
    static const char* const kt_name = NTAPS != 27 ? "igemm_fwd_kernel<flat>"
                                       : (TD * TH * TW == 512 ? "igemm_fwd_kernel<27,4x8x16>"
                                          : (TD * TH * TW == 128 ? "igemm_fwd_kernel<27,4x4x8>" : "igemm_fwd_kernel<27,2x4x8>"));
    MSSEG_KTIMED(kt_name, stream, hipLaunchKernelGGL(kern, grid, dim3(C::NTHREADS), lds, stream, p));
    MSSEG_CHECK_LAUNCH("igemm_fwd");
    if (EPI == EPI_STORE && p.fused.stats != nullptr)
        return msseg_k3_fused_finalize(p.fused, gx, p.N, C::COUTB, p.M, p.fused.nb_y != nullptr, ncb, stream);
    return MSSEG_OK;
}

template <typename T, int NTAPS, int SRC, int EPI, int TD, int TH, int TW, int WAVES, int STRIDE = 1>
int launch_nt(IgemmParams& p, hipStream_t stream) {
    const int cb = p.cout_block ? p.cout_block : msseg_cout_block(p.M);
    switch (cb) {
        case 16: return launch_cfg<T, NTAPS, SRC, EPI, TD, TH, TW, WAVES, 1, STRIDE>(p, stream);
        case 32: return launch_cfg<T, NTAPS, SRC, EPI, TD, TH, TW, WAVES, 2, STRIDE>(p, stream);
        case 48: return launch_cfg<T, NTAPS, SRC, EPI, TD, TH, TW, WAVES, 3, STRIDE>(p, stream);
    }
    MSSEG_FAIL(MSSEG_EINVAL, "igemm: bad cout block %d", cb);
}

// launch_nt of the 4x8x16 tile of conv k3, without the 48-wide (NT = 3) instantiation: it spilled (142 VGPRs) and cannot be
// reached.  The only caller of msseg_igemm_k3_big_* is launch_k3 (igemm_fwd.hip), which always sets p.cout_block from
// k3_plan, and k3_plan answers 32 in place of 48 whenever it picks this tile.  No other entry point leads to a 27-tap
// stride-1 instantiation.
template <typename T> int launch_k3_big(IgemmParams& p, hipStream_t stream) {
    switch (p.cout_block) {
        case 16: return launch_cfg<T, 27, SRC_DIRECT, EPI_STORE, 4, 8, 16, 8, 1>(p, stream);
        case 32: return launch_cfg<T, 27, SRC_DIRECT, EPI_STORE, 4, 8, 16, 8, 2>(p, stream);
    }
    MSSEG_FAIL(MSSEG_EINVAL, "igemm: bad cout block %d", p.cout_block);
}

// body of a family's msseg_igemm_* launcher: launch_nt for the run-time dtype (both dtypes, every cout block)
template <int NTAPS, int SRC, int EPI, int TD, int TH, int TW, int WAVES, int STRIDE = 1>
int launch_dtype(IgemmParams& p, int dtype, hipStream_t stream) {
    int rc = MSSEG_OK;
    const bool known = for_dtype(dtype, [&](auto t) {
        rc = launch_nt<typename decltype(t)::type, NTAPS, SRC, EPI, TD, TH, TW, WAVES, STRIDE>(p, stream);
    });
    if (!known) MSSEG_FAIL(MSSEG_EINVAL, "igemm: bad dtype %d", dtype);
    return rc;
}

}  // namespace
