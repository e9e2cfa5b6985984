// Tile-walking scaffolding shared by the persistent-workgroup 3x3x3 kernels: conv3d_k3_pp.hip, conv3d_k3_c48.hip,
// conv3d_k3_wgrad_pp.hip and stem_conv.hip.  What a kernel file still provides: its halo layout and the loads that fill it,
// its MFMA role, and the order of operations in its memory role.
//
// Everything here has internal linkage: the library is not built with relocatable device code, so a translation unit that
// includes this header gets its own copy (of the zero chunk in particular).
#pragma once
#include "common.h"

namespace {

// ---- tile schedule -----------------------------------------------------------------------------------------------
struct TileCo { int n, d0, h0, w0; };   // sample and first output voxel of a tile

// The persistent workgroup's walk over the TD x TH x TW tiles of an [N, D, H, W] grid: each XCD (workgroup id mod 8) walks
// one contiguous eighth of the tile list, so that neighbouring tiles, which share halo voxels, are fetched through the same
// L2 at about the same time; the cout blocks of one grid column share the XCD.  Tile k of this workgroup is tile(k), k < n_my.
template <int TD, int TH, int TW> struct Sched {
    int tiles_w, tiles_h, tiles_d, t_first, t_step, n_my;
    MSSEG_DEVFN void init(int N, int D, int H, int W) {
        tiles_w = (W + TW - 1) / TW; tiles_h = (H + TH - 1) / TH; tiles_d = (D + TD - 1) / TD;
        const int ntiles = N * tiles_d * tiles_h * tiles_w;
        int t_end;
        if ((gridDim.x & 7) == 0) {
            const int chunk = (ntiles + 7) >> 3, xcd = blockIdx.x & 7;
            t_first = xcd * chunk + (blockIdx.x >> 3);
            t_step = gridDim.x >> 3;
            t_end = min(ntiles, (xcd + 1) * chunk);
        } else {
            t_first = blockIdx.x; t_step = gridDim.x; t_end = ntiles;
        }
        n_my = t_first < t_end ? (t_end - t_first + t_step - 1) / t_step : 0;
    }
    MSSEG_DEVFN TileCo tile(int k) const {
        int t = t_first + k * t_step;
        TileCo tc;
        tc.w0 = (t % tiles_w) * TW; t /= tiles_w;
        tc.h0 = (t % tiles_h) * TH; t /= tiles_h;
        tc.d0 = (t % tiles_d) * TD; t /= tiles_d;
        tc.n = t;
        return tc;
    }
};

// ---- LDS-DMA --------------------------------------------------------------------------------------------------------
// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4); the LDS side is lane-linear
MSSEG_DEVFN void glds16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
__device__ u32x4_t g_zero_chunk;   // DMA source of padding voxels

// ---- transposing LDS reads through an LDS-address-space pointer -------------------------------------------------------
typedef __attribute__((address_space(3))) unsigned char lds_u8;
// the pointer stays an LDS-address-space pointer up to the builtin so that constant offsets fold into the
// instruction's 16-bit offset field (one address VGPR per lane-dependent base instead of one per read); common.h's
// lds_tr_read / tr_frag take a generic pointer plus register offsets
MSSEG_DEVFN bf16x4_t lds_tr(lds_u8* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)p);
}
MSSEG_DEVFN u32x4_t tr_frag(lds_u8* r0, lds_u8* r1) {
    const bf16x4_t lo = lds_tr(r0), hi = lds_tr(r1);
    const bf16x8_t f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(u32x4_t, f);
}

// ---- bf16 pairs and accumulation in the memory role ---------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
MSSEG_DEVFN unsigned pack_bf16x2(float a, float b) {            // one v_cvt_pk_bf16_f32 (round to nearest even)
    const bf16x2_t v = {(bf16_t)a, (bf16_t)b};
    return __builtin_bit_cast(unsigned, v);
}
MSSEG_DEVFN float bf16_of_pair(unsigned u, int hi) {            // element `hi` of a packed pair as f32: one shift / mask
    return __builtin_bit_cast(float, hi ? (u & 0xffff0000u) : (u << 16));
}
// plain v_add_f32 / v_fmac_f32: the compiler would pair the sums of neighbouring channels into packed-f32 instructions, which
// cost a wave that shares its SIMD with back-to-back MFMAs several issue slots each
MSSEG_DEVFN void acc_add(float& s, float v) { asm("v_add_f32 %0, %0, %1" : "+v"(s) : "v"(v)); }
MSSEG_DEVFN void acc_fma(float& s, float a, float b) { asm("v_fmac_f32 %0, %1, %2" : "+v"(s) : "v"(a), "v"(b)); }

// ---- fused-statistics epilogue --------------------------------------------------------------------------------------------
// Running (sum, sum2) of the current sample for the 4 consecutive couts a lane holds in each of its JT 16-wide cout tiles
// (lane = 16 * q + r: voxel r, couts 4q .. 4q+3): kept per lane across tiles, reduced over the 16 voxel lanes (fixed
// butterfly order) into this wave's private LDS slot when the sample changes and at the end; the 8 waves' slots are then
// added in a fixed order into the workgroup's partial row, which msseg_k3_fused_finalize sums over the workgroups:
// deterministic, no atomics.  NMAX = samples with a slot.  PLAIN_VALU (see acc_add) or the compiler's own choice of
// instructions for the sums; the values are the same, the kernels keep the form they were measured with.
template <int JT, int NMAX, bool PLAIN_VALU> struct StatAcc {
    static constexpr int WAVES = 8, CBW = JT * 16;
    static constexpr int LDS_FLOATS = WAVES * NMAX * CBW * 2;
    float s1[JT][4], s2[JT][4];
    int s_n;
    float* ldsS;
    int wave, r, q;

    MSSEG_DEVFN void init(float* lds, int wave_, int lane) {
        ldsS = lds; wave = wave_; r = lane & 15; q = lane >> 4;
        s_n = -1;
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) s1[j][e] = s2[j][e] = 0.f;
    }
    MSSEG_DEVFN void zero_slots() {   // all threads of the workgroup, before the barrier that ends the prologue
        for (int i = threadIdx.x; i < LDS_FLOATS; i += WAVES * 64) ldsS[i] = 0.f;
    }
    MSSEG_DEVFN void flush() {
        if (s_n < 0) return;
        float* slot = ldsS + ((wave * NMAX + s_n) * CBW) * 2;
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = s1[j][e], b = s2[j][e];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    a += __shfl_xor(a, o);
                    b += __shfl_xor(b, o);
                }
                if (r == 0) {
                    float* sp = slot + (j * 16 + q * 4 + e) * 2;
                    sp[0] += a;
                    sp[1] += b;
                }
                s1[j][e] = s2[j][e] = 0.f;
            }
    }
    MSSEG_DEVFN void sample(int n) {   // the tile about to be added belongs to sample n
        if (n != s_n) { flush(); s_n = n; }
    }
    MSSEG_DEVFN void add2(int j, int e, float a, float b, float c) {   // s1 += a, s2 += b * c
        if constexpr (PLAIN_VALU) {
            acc_add(s1[j][e], a);
            acc_fma(s2[j][e], b, c);
        } else {
            s1[j][e] += a;
            s2[j][e] += b * c;
        }
    }
    // forward: v = the value as stored
    MSSEG_DEVFN void add(int j, int e, float v) { add2(j, e, v, v, v); }
    // InstanceNorm-backward sums of the receiving layer: v = da as stored, av = its activation, yraw = its raw output;
    // dz = da * lrelu'(a); accumulates (sum dz, sum dz * yraw); xhat is formed by the finalising block
    MSSEG_DEVFN void add_inbwd(int j, int e, float v, float av, float slope, float yraw) {
        const float dz = v * (av > 0.f ? 1.0f : slope);
        add2(j, e, dz, dz, yraw);
    }
    // waves -> the workgroup's partial row ws[(blockIdx.y * gridDim.x + blockIdx.x) * N * CBW * 2 ..]
    MSSEG_DEVFN void finish(float* ws, int N) {
        flush();
        __syncthreads();
        const int PN = N * CBW * 2;
        float* wsp = ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * PN;
        for (int i = threadIdx.x; i < PN; i += WAVES * 64) {
            float s = 0.f;
#pragma unroll
            for (int wv = 0; wv < WAVES; ++wv) s += ldsS[wv * NMAX * CBW * 2 + i];
            wsp[i] = s;
        }
    }
};

}  // namespace
