// Ping-pong conv3d k3 kernel (bf16, 32 input channels per stage, 32-wide cout blocks): host-side interface.
#pragma once
#include "common.h"

// Operands of the reductions fused into a conv epilogue (all optional; stats == nullptr: none).  The kernel writes one
// partial row per workgroup to stats_ws, msseg_k3_fused_finalize adds the rows.
struct K3Fused {
    float* stats;        // per-(n, cout) (sum, sum of squares) of the stored output, [N][M][2]
    float* stats_ws;     // partial rows (the reduce scratch past its reserved header)
    long long nb_S;      // voxels per sample
    // InstanceNorm-BACKWARD sums (nb_y != nullptr): the launch produces da, the gradient w.r.t. the activation
    // a = lrelu(IN(yraw)); the epilogue accumulates (sum dz, sum dz * yraw), dz = da * lrelu'(a), and the finalise step
    // turns them into stats[n][c] = (sum dz, sum dz * xhat) and emits dbeta / dgamma
    const void* nb_y; long long nb_ldy;   // yraw
    const void* nb_a; long long nb_lda;   // a
    const float* nb_stats;                // [N][M][2] forward statistics (sum, sum of squares) of yraw
    float nb_slope, nb_eps;
    float* nb_dgamma; float* nb_dbeta; int nb_acc;
};
// Second step of the fused reductions (igemm_fwd.hip): one small block per cout block (and sample, forward) adds the gx
// partial rows ws[(y * gx + x) * N * coutb * 2 ..] of the ncb cout blocks in a fixed order and writes the per-(n, channel)
// results; inbwd: the InstanceNorm-backward form.  A separate launch: the kernel boundary makes the partial rows visible
// without release/acquire fences (which would write back / invalidate whole L2s at the end of every conv launch).
int msseg_k3_fused_finalize(const K3Fused& f, int gx, int N, int coutb, int M, bool inbwd, int ncb, hipStream_t stream);

// Workgroups per cout block (grid.x) of a persistent tile-walking kernel with per_cu workgroups per CU and ncb blocks in
// grid.y: a multiple of 8, so that the XCD-contiguous tile schedule applies, and at most one per tile
static inline int msseg_k3_grid_x(int per_cu, int ncb, long long tiles) {
    int gx = msseg_num_cus() * per_cu / ncb;
    gx &= ~7;
    if (gx < 8) gx = 8;
    if (gx > tiles) gx = (int)tiles;
    return gx;
}
// 4 x 4 x 16 output tiles of an [N, D, H, W] grid
static inline long long msseg_k3_tiles(int N, int D, int H, int W) {
    return (long long)N * ceil_div(D, 4) * ceil_div(H, 4) * ceil_div(W, 16);
}

// ---- generic implicit-GEMM forward kernel (igemm_fwd_kernel.h): one launcher per family, defined in the igemm_*.hip file
// that holds the family's instantiations; p.cout_block == 0 means msseg_cout_block(p.M).  Hidden: the split adds nothing
// to the library's exported symbols ----
struct IgemmParams;
#pragma GCC visibility push(hidden)
int msseg_igemm_k3_big_f32(IgemmParams& p, hipStream_t stream);            // 27 taps, 4x8x16 tiles; p.cout_block 16 or 32
int msseg_igemm_k3_big_bf16(IgemmParams& p, hipStream_t stream);
int msseg_igemm_k3_mid(IgemmParams& p, int dtype, hipStream_t stream);     // 27 taps, 4x4x8 tiles
int msseg_igemm_k3_small(IgemmParams& p, int dtype, hipStream_t stream);   // 27 taps, 2x4x8 tiles
int msseg_igemm_k3s2(IgemmParams& p, int dtype, hipStream_t stream);       // 27 taps, stride 2
int msseg_igemm_flat(IgemmParams& p, int dtype, hipStream_t stream);       // 1 tap: direct source, plain store
int msseg_igemm_gather(IgemmParams& p, int dtype, hipStream_t stream);     // 1 tap: im2col gather source
int msseg_igemm_deconv(IgemmParams& p, int dtype, hipStream_t stream);     // 1 tap: ConvTranspose k2 s2 scatter epilogue; cout block 32
int msseg_igemm_deconv_bwd(IgemmParams& p, int dtype, hipStream_t stream); // 1 tap: ConvTranspose k2 s2 children as source
#pragma GCC visibility pop

struct K3ppParams {
    const void* x;
    long long ldx;
    const void* wp;      // msseg_pack_weights image for cout block 32: [coutblk][kblk][27][4][32][16 B]
    const float* bias;   // optional
    void* y;
    long long ldy;
    int N, D, H, W, K, M;
    K3Fused fused;
    int accumulate;      // 1: y += conv(x) (the stored bf16 values are read back in the epilogue), statistics of the sums
    // split output (split_cb > 0; plain epilogue only): cout blocks [0, split_cb) go to (y, ldy) as always, blocks
    // [split_cb, M / 32) to (y2, ldy2) from its channel 0 -- two dense tensors instead of the two halves of one row
    void* y2;
    long long ldy2;
    int split_cb;
};

// true when the problem can run on the ping-pong kernel (otherwise the generic igemm kernel is used)
bool msseg_k3pp_eligible(const K3ppParams& p);
int msseg_k3pp_launch(const K3ppParams& p, hipStream_t stream);

// ---- 48 input channels per launch, 16-wide cout blocks (conv3d_k3_c48.hip); weight image = hip.pack_conv_k3_c48 ----
bool msseg_k3c48_shape_ok(int N, int D, int H, int W, int M);   // grid / channel conditions (what the packer must know)
bool msseg_k3c48_eligible(const K3ppParams& p);                 // ... and operand alignment
int msseg_k3c48_launch(const K3ppParams& p, hipStream_t stream);

// ---- weight gradient (conv3d_k3_wgrad_pp.hip) ----
struct K3WgParams {
    const void* pten; long long ldp;   // dy (channels M)
    const void* qten; long long ldq;   // x  (channels K)
    float* slabs;                      // [pair = mblk * kblks + kblk][workgroup][27][32][32] fp32 partial sums
    int N, D, H, W, M, K, kblks;
};
bool msseg_k3wg_pp_eligible(const K3WgParams& p);
int msseg_k3wg_pp_grid(const K3WgParams& p);      // workgroups per block pair (= slabs per pair)
int msseg_k3wg_pp_launch(const K3WgParams& p, int gx, hipStream_t stream);

// ---- one-input-channel stem convolution (stem_conv.hip) ----
struct StemParams {
    const void* x; long long ldx;     // [N, D, H, W, 1] bf16
    const void* wp;                   // packed image, K = 27, cout block 32
    const float* bias;
    void* y; long long ldy;
    int N, D, H, W, M;
    float* stats; float* stats_ws;    // optional fused statistics (partial rows -> msseg_k3_fused_finalize)
    int taps;                         // 27 (or 0): conv k3 p1; 1: the 1x1x1 conv of a one-channel volume (image with K = 1)
    // y == nullptr (with stats): statistics only, nothing is stored.  nstats != nullptr: y = lrelu(instance_norm(conv) * gamma +
    // beta) with the statistics nstats[N][M][2] of a previous statistics-only launch (inference: the raw output never exists)
    const float* nstats; const float* gamma; const float* beta; float eps, slope;
};
struct StemWgParams {
    const void* x; long long ldx;
    const void* dy; long long lddy;
    float* slabs;                     // [cout block][workgroup][32][32] fp32
    int N, D, H, W, M;
    // yraw != nullptr (dy unused): dy = the InstanceNorm + LeakyReLU backward apply of (yraw, da) with the forward statistics
    // stats[N][M][2] and the backward sums red[N][M][2], formed tile by tile and never stored; N <= 8
    const void* yraw; long long ldyraw;
    const void* da; long long ldda;
    const float* stats; const float* red; const float* gamma; const float* beta; float eps, slope;
};
bool msseg_stem_eligible(int dtype, int Cin, int Cout, int k, int s, int pd, long long ldx, long long ldy, const void* y);
int msseg_stem_fwd_launch(const StemParams& p, hipStream_t stream);
int msseg_stem_wgrad_grid(const StemWgParams& p);
int msseg_stem_wgrad_launch(const StemWgParams& p, int gx, hipStream_t stream);

// ---- ConvTranspose3d k2 s2, register-resident weights (deconv_k2s2.hip) ----
bool msseg_deconv2_fast_eligible(int dtype, int Cin, int Cout, const void* coarse, long long ldc, const void* fine,
                                 long long ldf, const float* bias);
int msseg_deconv2_fwd_launch(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy, int N,
                             int D, int H, int W, int Cin, int Cout, hipStream_t stream);
int msseg_deconv2_bwd_launch(const void* dy, long long lddy, const void* wp, void* dx, long long lddx, int N, int D, int H,
                             int W, int Cin, int Cout, const void* yraw, long long ldyraw, const void* act, long long ldact,
                             const float* fwd_stats, float slope, float eps, float* red, float* dgamma, float* dbeta,
                             int accumulate, float* dbias, int dbias_accumulate, void* scratch, size_t scratch_bytes,
                             hipStream_t stream);

// ---- ConvTranspose3d k2 s2 for any channel count with an instantiation, output sliced over grid.y (deconv_k2s2_gen.hip) ----
bool msseg_deconv2g_fwd_eligible(int dtype, int Cin, int Cout, const void* coarse, long long ldc, const void* fine,
                                 long long ldf, const float* bias);
int msseg_deconv2g_fwd_launch(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy, int N,
                              int D, int H, int W, int Cin, int Cout, hipStream_t stream);
bool msseg_deconv2g_bwd_eligible(int dtype, int Cin, int Cout, const void* coarse, long long ldc, const void* fine,
                                 long long ldf);
int msseg_deconv2g_bwd_launch(const void* dy, long long lddy, const void* wp, void* dx, long long lddx, float* part, int N,
                              int D, int H, int W, int Cin, int Cout, hipStream_t stream);
// ---- Linear / 1x1x1 conv on many tokens with few channels, register-resident weights (linear_regw.hip) ----
bool msseg_linear_regw_eligible(int dtype, long long NV, int Cin, int Cout, const void* x, long long ldx, const void* y,
                                long long ldy, const float* bias);
int msseg_linear_regw_launch(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                             long long NV, int Cin, int Cout, hipStream_t stream);
