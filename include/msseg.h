/* msseg.h -- C ABI of libmsseg_hip.so: the MI355X (gfx950) kernels behind the 3-D segmentation
 * hot path (UNet / Swin-UNETR forward+backward, Dice+CE loss, sliding-window blend).
 *
 * The reference (zouyunkai/MedicalSemSeg) has no FFI layer: its hot path is torch/ATen + MONAI calls
 * issued from Python.  Each entry point below names the reference call site(s) whose arithmetic it
 * replaces (paths relative to /root/reference).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - All tensors are dense "channels-last" volumes [N, D, H, W, C]; `ld*` is the element distance
 *    between consecutive voxels (>= C), so a kernel can read/write a channel slice of a wider
 *    (concatenated) buffer.  Pointers must be 16-byte aligned and ld*sizeof(elem) a multiple of 16.
 *  - dtype: MSSEG_F32 (exact fp32 MFMA path, used for parity) or MSSEG_BF16 (bf16 storage, fp32
 *    accumulate).  Reductions, statistics, weight gradients and losses are always fp32.
 *  - Every call only ENQUEUES work on `stream` (a hipStream_t); it never allocates, frees, syncs or
 *    keeps caller pointers.  Scratch comes from the caller (`workspace`), sized by the *_workspace_bytes
 *    queries.  Safe to capture into a hipGraph.
 *  - Return value: MSSEG_OK or a negative MSSEG_E* code; msseg_last_error() gives a thread-local message.
 */
#ifndef MSSEG_H_
#define MSSEG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSSEG_ABI_VERSION 3

#define MSSEG_OK 0
#define MSSEG_EINVAL (-1)   /* bad argument / unsupported shape */
#define MSSEG_ELAUNCH (-2)  /* HIP launch error */
#define MSSEG_EWORKSPACE (-3) /* workspace too small */

#define MSSEG_F32 0
#define MSSEG_BF16 1

typedef void* msseg_stream_t; /* hipStream_t */

int msseg_abi_version(void);
const char* msseg_last_error(void);
/* number of compute units of the current device (grid sizing of the persistent kernels) */
int msseg_num_cus(void);

/* Measurement aid (no reference counterpart): while enabled, the launches of the main convolution kernels (k3pp_kernel,
 * k3wg_pp_kernel, igemm_fwd_kernel, igemm_wgrad_kernel) are bracketed by a hipEvent pair on their stream; `_get` returns
 * the kernel's name and the elapsed time of record i (it waits for that launch).  Process-wide, not for use while a
 * stream is capturing.  bench.py derives `roofline.achieved` of the dominant kernel from these. */
int msseg_ktimer_enable(int on);
int msseg_ktimer_reset(void);
int msseg_ktimer_count(void);
int msseg_ktimer_get(int i, char* name, int cap, float* ms);

/* ---------------------------------------------------------------------------------------------
 * Weight packing.  Source: fp32 parameter in torch layout.  Destination: the MFMA operand image
 * [cout_block][k_block][tap][quarter][cout_in_block][16 bytes] consumed by the igemm kernels.
 * Logical matrix W[m][t][k], m = m1*M0+m0, k = k1*K0+k0, read from
 *   src[m1*s_m1 + m0*s_m0 + t'*s_t + k1*s_k1 + k0*s_k0],  t' = flip ? T-1-t : t.
 * ------------------------------------------------------------------------------------------- */
size_t msseg_packed_weight_bytes(int M, int T, int K, int cout_block, int dtype);
int msseg_pack_weights(const float* src, void* dst, int dtype, int M, int M0, int T, int K, int K0,
                       long long s_m1, long long s_m0, long long s_t, long long s_k1, long long s_k0,
                       int flip, int cout_block, msseg_stream_t stream);
/* Batched form: one launch repacks every job of a device-resident table (all jobs share `dtype`).  Used once per
 * optimizer step to refresh all packed images of a network (reference equivalent: none -- torch.nn.Conv3d reads the
 * fp32 parameter directly, /root/reference/run_training.py:92-93 updates it in place). */
typedef struct msseg_pack_job {
    const float* src;
    void* dst;
    long long s_m1, s_m0, s_t, s_k1, s_k0;
    long long total;          /* elements of the destination image = msseg_packed_weight_bytes / element size */
    int M, M0, T, K, K0, flip, cout_block, nkb;   /* nkb = ceil(K / (64 / element size)) */
} msseg_pack_job;
/* max_total / sum_total: largest and summed `total` of the table's jobs (the table itself is device memory: the grid is sized
 * from these) */
int msseg_pack_weights_batch(const msseg_pack_job* jobs_dev, int njobs, long long max_total, long long sum_total, int dtype,
                             msseg_stream_t stream);
/* cout block (16/32/48) the igemm kernels use for a layer with M logical output channels */
int msseg_cout_block(int M);
/* cout block msseg_conv3d_k3_fwd will use for this problem (pack the weights with it) */
int msseg_conv3d_k3_cout_block(int N, int D, int H, int W, int Cout);
/* tile variant it will use: 0 = 4x8x16-voxel tiles / 8 waves (the MFMA-bound large layers), 1 = 4x4x8, 2 = 2x4x8 */
int msseg_conv3d_k3_variant(int N, int D, int H, int W, int Cout);
/* kernel msseg_conv3d_k3_fwd / _dgrad_inbwd will run for this problem (16-byte aligned, dense operands):
 * 0/1/2 = generic implicit-GEMM tile configurations (as msseg_conv3d_k3_variant), 3 = the LDS-DMA ping-pong kernel
 * (bf16, 32 input channels per stage, large grids), 4 = the 48-input-channel ping-pong kernel (bf16, Cin == 48,
 * Cout % 16 == 0, N <= 4, large grids: Swin-UNETR's 48-wide UnetResBlock convolutions, models/segmentors/swin_unetr.py:
 * 73-128).  Variant 4 reads a DIFFERENT weight image -- four msseg_pack_weights images back to back, see
 * medicalsemseg_amd/hip.py pack_conv_k3_c48 and csrc/conv3d_k3_c48.hip -- so the packer must ask this function. */
int msseg_conv3d_k3_kernel(int N, int D, int H, int W, int Cin, int Cout, int dtype);
/* Workgroups of that kernel the runtime keeps resident on one CU, at the dynamic LDS size the launcher passes for a batch of N
 * (the generic kernel's statistics area is sized by N).  Generic variants 0/1/2 only: MSSEG_EINVAL where
 * msseg_conv3d_k3_kernel answers 3 or 4.  Needs a device; launches nothing.  MSSEG_K3_MID_ONE_PER_CU=1 in the environment
 * (read once) makes the 4x4x8 tile pass its full-size area again: one workgroup per CU with the same code. */
int msseg_conv3d_k3_resident_per_cu(int N, int D, int H, int W, int Cin, int Cout, int dtype);

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM convolutions (forward-shaped).  y = conv(x, W) + bias.
 * ------------------------------------------------------------------------------------------- */
/* Conv3d k=3 s=1 p=1.  Replaces nn.Conv3d 3x3x3 inside MONAI UnetResBlock / BasicUNet TwoConv
 * (models/segmentors/swin_unetr.py:73-128) and, with dgrad-packed weights, its input gradient.
 * Requires Cin % (16/sizeof(elem)) == 0. */
int msseg_conv3d_k3_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                        int N, int D, int H, int W, int Cin, int Cout, float* stats /* nullable: fused InstanceNorm
                        statistics stats[n][cout][2] = (sum, sum of squares) of y as stored; needs N <= 8 */,
                        void* scratch, size_t scratch_bytes, int dtype, msseg_stream_t stream);
/* Input gradient of a conv k3 (dgrad-packed weights) FUSED with the InstanceNorm-backward reductions of the layer
 * whose activation receives that gradient: da = conv(dy, W'); red[n][c] = (sum dz, sum dz*xhat) with
 * dz = da*lrelu'(act), xhat from (yraw, fwd_stats); dbeta/dgamma (nullable) = sum_n red (written or accumulated).
 * Saves the separate msseg_instnorm_act_bwd_reduce pass (3 tensor reads).  N <= 8, Cout % 4 == 0. */
/* y += conv3d k3 (x, w) without bias: the stored bf16 values of y are read back and the sums stored; stats = InstanceNorm
 * statistics of the sums.  Lets a 64-input-channel layer over cat([a, b]) run as two 32-channel launches on the ping-pong
 * kernel without a concat buffer (inference forward of MONAI BasicUNet's UpCat convs).  Only for shapes the
 * ping-pong kernel takes (bf16, Cin == 32, Cout % 32 == 0, large grids: msseg_conv3d_k3_kernel() == 3), and with
 * Cin == 48 for the shapes of the 48-channel kernel (== 4): a 96-input-channel layer over cat([up, skip]) as two launches
 * on the channel halves of the concat buffer (ldx = 96), Swin-UNETR's decoder blocks. */
int msseg_conv3d_k3_fwd_accumulate(const void* x, long long ldx, const void* wp, void* y, long long ldy, int N, int D, int H,
                                   int W, int Cin, int Cout, float* stats, void* scratch, size_t scratch_bytes, int dtype,
                                   msseg_stream_t stream);
/* Conv3d k=3 s=1 p=1 with TWO destinations: output channels [0, split) go to (y, ldy), channels [split, Cout) to (y2, ldy2)
 * from its channel 0.  For the input gradient of a conv over cat([a, b]) (BasicUNet's UpCat convs): the gradients of a and b
 * come out as two dense tensors, so that their readers fetch whole cache lines instead of half rows of one 2 x 32-channel
 * tensor.  Same values as msseg_conv3d_k3_fwd, element for element.  Only for problems msseg_conv3d_k3_split_ok accepts
 * (the ping-pong kernel, split on a 32-channel boundary) and only with the plain epilogue: stats != NULL or accumulate != 0
 * is MSSEG_EINVAL, as is any other problem -- there is no second implementation on the generic kernels. */
int msseg_conv3d_k3_fwd_split(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                              void* y2, long long ldy2, int split, int N, int D, int H, int W, int Cin, int Cout,
                              float* stats, int accumulate, int dtype, msseg_stream_t stream);
/* 1 if msseg_conv3d_k3_fwd_split takes this problem (16-byte aligned, dense operands): it runs on the ping-pong kernel
 * (msseg_conv3d_k3_kernel() == 3), Cout % 32 == 0, 0 < split < Cout and split % 32 == 0; 0 otherwise */
int msseg_conv3d_k3_split_ok(int N, int D, int H, int W, int Cin, int Cout, int split, int dtype);
int msseg_conv3d_k3_dgrad_inbwd(const void* dy, long long lddy, const void* wp, void* da, long long ldda, int N, int D,
                                int H, int W, int Cin, int Cout, const void* yraw, long long ldyraw, const void* act,
                                long long ldact, const float* fwd_stats, float slope, float eps, float* red,
                                float* dgamma, float* dbeta, int accumulate, void* scratch, size_t scratch_bytes,
                                int dtype, msseg_stream_t stream);
/* Conv3d k=3 s=2 p=1 (PatchMerging.reduction, models/backbones/swin_nnformer.py:297): x [N,ID,IH,IW,Cin] ->
 * y [N,(ID-1)/2+1,...,Cout].  Its input / weight gradients run as stride-1 problems on msseg_zero_stuff2(dy). */
int msseg_conv3d_k3s2_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                          int N, int ID, int IH, int IW, int Cin, int Cout, int dtype, msseg_stream_t stream);
int msseg_zero_stuff2(const void* dy, long long lddy, void* out, long long ldo, int N, int OD, int OH, int OW, int ID,
                      int IH, int IW, int C, int dtype, msseg_stream_t stream);
/* Conv3d k=3 s=1 p=1 with ONE input channel (BasicUNet conv_0.conv_0, the stem): dedicated kernel, bf16, Cout % 32 == 0 or
 * % 48 == 0 (Swin-UNETR's 1 -> 48 first conv); y == NULL with stats != NULL: statistics only, nothing is stored;
 * wp = the msseg_pack_weights image used by msseg_conv3d_gather_fwd (K = 27); optional fused statistics as
 * msseg_conv3d_k3_fwd.  k = 3, or k = 1: the 1x1x1 convolution of a one-channel volume (UnetResBlock conv3 of Swin-UNETR's
 * encoder1; wp = the gather image with K = 1) on the same kernel, centre tap only; any other k is MSSEG_EINVAL.
 * msseg_conv3d_gather_fwd / _wgrad route eligible problems here by themselves; this entry point adds the statistics.
 * Returns MSSEG_EINVAL for problems the stem kernel does not cover. */
int msseg_conv3d_stem_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                          int N, int D, int H, int W, int Cout, int k, float* stats, void* scratch, size_t scratch_bytes,
                          int dtype, msseg_stream_t stream);
/* Inference form of the stem unit: y = lrelu(instance_norm(conv(x) + bias) * gamma + beta) with the statistics stats[N][Cout][2]
 * of a statistics-only msseg_conv3d_stem_fwd call in front -- the one-channel conv is cheap enough to run twice, and the raw
 * output's write and the normalisation pass over it disappear (sliding-window inference of BasicUNet at 96^3 windows). */
int msseg_conv3d_stem_norm_fwd(const void* x, long long ldx, const void* wp, const float* bias, const float* stats,
                               const float* gamma, const float* beta, float eps, float slope, void* y, long long ldy, int N,
                               int D, int H, int W, int Cout, int dtype, msseg_stream_t stream);
/* Conv3d k=1 (UnetResBlock.conv3, UnetOutBlock models/segmentors/swin_unetr.py:130, BasicUNet final_conv). */
int msseg_conv3d_k1_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                        long long NV, int Cin, int Cout, int dtype, msseg_stream_t stream);
/* The same for a segmentation head with 1..4 output channels (UnetOutBlock / final_conv with 2-4 classes): a streaming
 * kernel, w = the layer's fp32 weight [Cout][Cin] as it is (no packed image), Cin <= 64 in 16-byte chunks.
 * MSSEG_EINVAL for other shapes (use msseg_conv3d_k1_fwd). */
int msseg_conv3d_k1_head_fwd(const void* x, long long ldx, const float* w, const float* bias, void* y, long long ldy,
                             long long NV, int Cin, int Cout, int dtype, msseg_stream_t stream);
/* The head reading the RAW conv output `x` of the last conv + InstanceNorm + LeakyReLU unit (N samples of S voxels):
 * y = conv1x1(T(lrelu(IN(x) * gamma + beta))) with the normalisation applied in registers -- the unit's activation is
 * never written.  stats: [N][Cin][2] (sum, sum of squares) of x.  Replaces InstanceNorm3d + LeakyReLU + final Conv3d(k=1)
 * of MONAI BasicUNet (TwoConv tail + final_conv). */
int msseg_conv3d_k1_head_norm_fwd(const void* x, long long ldx, const float* stats, const float* gamma, const float* beta,
                                  float slope, float eps, const float* w, const float* bias, void* y, long long ldy, int N,
                                  long long S, int Cin, int Cout, int dtype, msseg_stream_t stream);
/* The head's backward in one streaming pass.  Its input gradient fused with the InstanceNorm-backward sums of the layer
 * that feeds the head (as msseg_conv3d_k1_dgrad_inbwd, same streaming form): da[v][c] = sum_k dy[v][k] * w[k][c] for the C
 * channels of that layer, red[n][c] = (sum dz, sum dz*xhat) with the LeakyReLU sign recomputed from yraw (gamma, beta
 * nullable), dgamma/dbeta written or accumulated.  dy rows 16-byte aligned with >= 4 readable channels (classes
 * zero-padded).  dw (nullable: no weight gradient): dw[Cout][C] (+)= sum_v dy[v][k] * a[v][c] with the activation a
 * recomputed from yraw (as the fused forward does).  da == NULL (dw given): da is not stored. */
int msseg_conv3d_k1_head_bwd_fused(const void* dy, long long lddy, const float* w, void* da, long long ldda, int N,
                                   long long S, int C, int Cout, const void* yraw, long long ldyraw, const float* fwd_stats,
                                   const float* gamma, const float* beta, float slope, float eps, float* red, float* dgamma,
                                   float* dbeta, int accumulate, float* dw, int dw_accumulate, void* scratch,
                                   size_t scratch_bytes, int dtype, msseg_stream_t stream);

/* Conv3d with few input channels (Cin*k^3 <= 128), kernel k, stride s, pad p, gathered im2col-style:
 * the 1->C stem convs and PatchEmbed3D.proj (models/blocks/patch_embeddings.py:109). */
int msseg_conv3d_gather_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                            int N, int ID, int IH, int IW, int Cin, int Cout, int k, int s, int p, int dtype,
                            msseg_stream_t stream);
/* ConvTranspose3d k=s=2 (UnetrUpBlock.transp_conv, BasicUNet UpCat): x [N,D,H,W,Cin] -> y [N,2D,2H,2W,Cout]. */
int msseg_deconv_k2s2_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                          int N, int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream);
/* input gradient of the above: dy [N,2D,2H,2W,Cout] -> dx [N,D,H,W,Cin]. */
int msseg_deconv_k2s2_bwd_data(const void* dy, long long lddy, const void* wp, void* dx, long long lddx,
                               int N, int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream);
/* ConvTranspose3d k=s=4 (the last UnetrUpBlock.transp_conv of Swin-UNETR with patch size 4; csrc/deconv_k4s4.hip):
 * x [N,D,H,W,Cin] -> y [N,4D,4H,4W,Cout], y[n,4d+a,4h+b,4w+c,co] = bias[co] + sum_ci x[n,d,h,w,ci] * W[ci,co,a,b,c].
 * wp: msseg_pack_weights image with T = 1 -- forward: M = abc * Cout + co (abc = (a*4 + b)*4 + c), K = ci; input gradient:
 * M = ci, K = abc * Cout + co (hip.pack_deconv builds both).  ldx / ldy: voxel strides, so y may be the first Cout channels
 * of a concat buffer.  bf16 with Cin = Cout in {32, 48, 64, 96} (forward: Cin <= 96 a multiple of 8, Cout a multiple of 32 or
 * 48) and 16-byte aligned rows runs on MFMA kernels; fp32 and every other channel count on plain vector kernels.  All
 * three are deterministic (fixed-order reductions, no atomics). */
int msseg_deconv_k4s4_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                          int N, int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream);
/* input gradient of the above: dy [N,4D,4H,4W,Cout] -> dx [N,D,H,W,Cin]. */
int msseg_deconv_k4s4_bwd_data(const void* dy, long long lddy, const void* wp, void* dx, long long lddx,
                               int N, int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream);
/* The flat 1x1x1 input-gradient kernel with the InstanceNorm-backward sums of the RECEIVING layer fused into the epilogue
 * (arguments as msseg_conv3d_k3_dgrad_inbwd): the gradient that reaches the second conv+norm unit of a UNet level comes
 * from the 1x1x1 output conv (level 0) or from a transposed conv (other decoder levels / the bottleneck:
 * msseg_deconv_k2s2_bwd_fused below).  dy [N*S, Cin] -> da [N*S, Cout], S voxels per sample. */
int msseg_conv3d_k1_dgrad_inbwd(const void* dy, long long lddy, const void* wp, void* da, long long ldda, int N,
                                long long S, int Cin, int Cout, const void* yraw, long long ldyraw, const void* act,
                                long long ldact, const float* fwd_stats, float slope, float eps, float* red,
                                float* dgamma, float* dbeta, int accumulate, void* scratch, size_t scratch_bytes,
                                int dtype, msseg_stream_t stream);
/* Input gradient of ConvTranspose3d k2 s2 with everything the pass over dy can produce: dx, optionally (yraw != NULL) the
 * InstanceNorm-backward sums red[N][Cin][2] (+ dgamma / dbeta) of the layer that receives dx, and optionally
 * (dbias != NULL) the bias gradient dbias[Cout] (+)= sum over all fine voxels of dy.  bf16 layers with Cin in {32, 64},
 * Cout = 32 run on the register-resident-weight kernel (deconv_k2s2.hip): one read of dy, no statistics / channel-sum
 * passes; other shapes fall back to the implicit-GEMM kernel plus a channel-sum pass. */
int msseg_deconv_k2s2_bwd_fused(const void* dy, long long lddy, const void* wp, void* dx, long long lddx, int N,
                                int D, int H, int W, int Cin, int Cout, const void* yraw, long long ldyraw,
                                const void* act, long long ldact, const float* fwd_stats, float slope, float eps,
                                float* red, float* dgamma, float* dbeta, int accumulate, float* dbias, int dbias_accumulate,
                                void* scratch, size_t scratch_bytes, int dtype, msseg_stream_t stream);

/* Input gradient of ConvTranspose3d k2 s2 as ONE fp32 stage group in the layout of msseg_conv3d_k3_small_partials
 * (part[Cin / 4][N*D*H*W][4], csrc/deconv_k2s2_gen.hip): msseg_conv3d_k3_small_bwd_finish(part, 1, ...) then stores dx, or
 * runs the whole backward of the conv + InstanceNorm + LeakyReLU unit whose activation the transposed conv read (the deep
 * UpCat levels of MONAI BasicUNet; /root/reference/models/segmentors/swin_unetr.py:93-128 transp_conv).  bf16; dy: fine
 * [N, 2D, 2H, 2W, Cout]; wp: the backward image of msseg_pack_weights (M = Cin, K = 8 * Cout); part_bytes >= N*D*H*W*Cin*4.
 * msseg_deconv_k2s2_bwd_partials_ok() == 1 for the channel counts with an instantiation (Cin % 32 == 0, Cout / 16 in
 * {3, 4, 6, 8, 12, 24}). */
int msseg_deconv_k2s2_bwd_partials_ok(int Cin, int Cout, int dtype);
int msseg_deconv_k2s2_bwd_partials(const void* dy, long long lddy, const void* wp, float* part, size_t part_bytes, int N,
                                   int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * Weight gradients (fp32 output in the torch parameter layout; deterministic two-stage reduction).
 * `accumulate` != 0 adds into dw instead of overwriting.
 * ------------------------------------------------------------------------------------------- */
size_t msseg_wgrad_workspace_bytes(int M, int T, int K);
/* which kernel msseg_conv3d_k3_wgrad selects for dense (ld == channels), aligned tensors of this shape:
 * 3 = LDS-DMA ping-pong kernel (conv3d_k3_wgrad_pp.hip), 0 = generic igemm_wgrad kernel (tests assert the selection). */
int msseg_conv3d_k3_wgrad_kernel(int N, int D, int H, int W, int Cin, int Cout, int dtype);
int msseg_conv3d_k3_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw,
                          int N, int D, int H, int W, int Cin, int Cout, int accumulate,
                          void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream);
int msseg_conv3d_k1_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw,
                          long long NV, int Cin, int Cout, int accumulate,
                          void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream);
/* Weight AND bias gradient of nn.Linear / a 1x1x1 convolution in one pass over the tokens: dw[Cout][Cin] (+)= dy^T x,
 * dbias[Cout] (+)= column sums of dy (dbias nullable).  Replaces autograd's two reductions for the Swin stages' Linear layers
 * (models/backbones/swin_nnformer.py:24-42,128-196).  bf16; channel counts that split into the kernel's output slices
 * (msseg_linear_wgrad_ok() == 1: multiples of 48 on both sides cover every Swin width); deterministic; workspace as
 * msseg_wgrad_workspace_bytes(Cout, 1, Cin).  Callers keep msseg_conv3d_k1_wgrad + msseg_channel_sum otherwise. */
int msseg_linear_wgrad_ok(long long NV, int Cin, int Cout, int dtype);
int msseg_linear_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw, float* dbias, long long NV,
                       int Cin, int Cout, int accumulate_w, int accumulate_b, void* workspace, size_t workspace_bytes,
                       int dtype, msseg_stream_t stream);
int msseg_conv3d_gather_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw,
                              int N, int ID, int IH, int IW, int Cin, int Cout, int k, int s, int p, int accumulate,
                              void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream);
/* Weight gradient of the one-input-channel stem conv (k 3 p 1, or k 1) whose output feeds InstanceNorm + LeakyReLU, with
 * that unit's backward apply folded into the operand load: dy = apply(yraw, da; stats, red, gamma, beta) as
 * msseg_instnorm_act_bwd_apply (y = NULL) would store it is formed tile by tile and never written; dw has the bits of that
 * call followed by msseg_conv3d_gather_wgrad.  bf16, Cout a multiple of 32 or 48 (<= 256), N <= 8; anything else is an
 * error.  workspace as for msseg_conv3d_gather_wgrad. */
int msseg_conv3d_stem_wgrad_inbwd(const void* x, long long ldx, const void* yraw, long long ldyraw, const void* da,
                                  long long ldda, const float* stats, const float* red, const float* gamma, const float* beta,
                                  float eps, float slope, float* dw, int N, int D, int H, int W, int Cout, int k,
                                  int accumulate, void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream);
int msseg_deconv_k2s2_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw,
                            int N, int D, int H, int W, int Cin, int Cout, int accumulate,
                            void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream);
/* dw [Cin][Cout][4][4][4] (+)= sum over coarse voxels of x[v][ci] * dy[child abc of v][co] (ConvTranspose3d k4 s4);
 * workspace: at least Cin * 64 * Cout * 4 bytes (one partial image; more lets more workgroups share the voxels),
 * msseg_wgrad_workspace_bytes(Cin, 1, 64 * Cout) is ample. */
int msseg_deconv_k4s4_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw,
                            int N, int D, int H, int W, int Cin, int Cout, int accumulate,
                            void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * conv3d k3 s1 p1 on SMALL grids (12^3 / 6^3 levels of the UNet; csrc/conv3d_k3_small.hip), bf16: the 32-channel stages of a
 * layer are split over workgroups (split-K), the fp32 partial blocks part[stage group][Cout/4][N*D*H*W][4] are combined by a finish
 * kernel that also does what follows the conv -- forward: bias, bf16 raw output, InstanceNorm statistics, normalise +
 * LeakyReLU, optional 2x2x2 max-pool (MONAI TwoConv / Down); input gradient: either the plain sum, or the
 * whole backward of the conv + InstanceNorm + LeakyReLU unit whose activation was the conv's input (dy of that unit, its
 * dgamma / dbeta).  wp: msseg_pack_weights image with cout block 32 (forward image, or the flipped / transposed input-
 * gradient image).  D a multiple of 6 (3 for the tiles, even for the pool), H, W multiples of 6, D*H*W <= 2048; channels
 * multiples of 32; N <= 8.
 * ------------------------------------------------------------------------------------------- */
int msseg_conv3d_k3_small_ok(int N, int D, int H, int W, int Cin, int Cout, int dtype);
/* number of partial blocks per output element the partials call writes (= `nstages` of the finish calls) */
int msseg_conv3d_k3_small_stage_groups(int N, int D, int H, int W, int Cin, int Cout);
size_t msseg_conv3d_k3_small_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout);
int msseg_conv3d_k3_small_partials(const void* x, long long ldx, const void* wp, float* part, size_t part_bytes, int N,
                                   int D, int H, int W, int Cin, int Cout, msseg_stream_t stream);
/* residual (nullable, voxel stride ldr) is added before the LeakyReLU: act = lrelu(instance_norm(y) * gamma + beta +
 * residual) -- the second convolution of MONAI's UnetResBlock (models/segmentors/swin_unetr.py:73-128 of the reference) */
int msseg_conv3d_k3_small_fwd_finish(const float* part, int nstages, const float* bias, const float* gamma,
                                     const float* beta, float eps, float slope, void* yraw, long long ldy, void* act,
                                     long long lda, const void* residual, long long ldr, void* pooled, long long ldp,
                                     float* stats, int N, int D, int H, int W, int Cout, msseg_stream_t stream);
int msseg_conv3d_k3_small_bwd_finish(const float* part, int nstages, void* dx, long long lddx, const void* unit_yraw,
                                     long long lduy, const float* unit_stats, const float* unit_gamma,
                                     const float* unit_beta, float eps, float slope, float* dgamma, float* dbeta,
                                     int accumulate, int N, int D, int H, int W, int Cin, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depthwise Conv3d k3 s1 p1 (groups = channels) of the SwinDepth MLP (models/backbones/swindepth.py:36-41,56-65).
 * x, y channels-last [N, D, H, W, C] (C % (16 / sizeof(elem)) == 0); w_taps = the weight [C, 1, 3, 3, 3] transposed to
 * tap-major [27][C] in the tensors' dtype; flip = 1 mirrors the taps (the input gradient: dx = dwconv(dy, flip)).
 * wgrad: dw (torch layout [C, 1, 3, 3, 3], fp32) and dbias [C] written or accumulated; partial rows in `scratch`
 * (msseg_reduce_scratch_bytes()), added in row order by a second kernel -- deterministic.
 * ------------------------------------------------------------------------------------------- */
int msseg_dwconv3d_k3_fwd(const void* x, long long ldx, const void* w_taps, const float* bias, void* y, long long ldy, int N,
                          int D, int H, int W, int C, int flip, int dtype, msseg_stream_t stream);
/* nn.AvgPool3d(kernel_size=3, stride=1, padding=1), count_include_pad (models/backbones/swinception.py:113-116): the same
 * kernel with unit taps, the fp32 sum scaled by 1/27 before the one rounding to the tensors' dtype; self-adjoint. */
int msseg_avgpool3d_k3(const void* x, long long ldx, void* y, long long ldy, int N, int D, int H, int W, int C, int dtype,
                       msseg_stream_t stream);
int msseg_dwconv3d_k3_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw, float* dbias,
                            int accumulate_w, int accumulate_b, int N, int D, int H, int W, int C, void* scratch,
                            size_t scratch_bytes, int dtype, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depthwise Conv3d with an odd kernel K in {3, 5, 7, 9, 11}, stride 1, padding K / 2, groups = channels, no bias: the focal
 * convolutions of FocalNet (models/backbones/focalnet_3d.py:73-81).  x, y channels-last [N, D, H, W, C] with voxel strides
 * ldx / ldy (a channel slice of a wider buffer is fine), C % 8 == 0 for both dtypes, any D, H, W >= 1.  w_taps = the weight
 * [C, 1, K, K, K] transposed to tap-major [K^3][C] in the tensors' dtype; flip = 1 mirrors the taps (the input gradient).
 * fp32 accumulation.  Any other K or C returns MSSEG_EINVAL.
 * wgrad: dw (torch layout [C, 1, K, K, K], fp32) written or accumulated; partial rows in `workspace`
 * (msseg_dwconv3d_wgrad_workspace_bytes; a smaller one, down to one row of K^3 * C floats, is used as far as it goes) are
 * added in row order by a second kernel -- deterministic, no atomics.
 * ------------------------------------------------------------------------------------------- */
int msseg_dwconv3d_fwd(const void* x, long long ldx, const void* w_taps, void* y, long long ldy, int N, int D, int H, int W,
                       int C, int K, int flip, int dtype, msseg_stream_t stream);
size_t msseg_dwconv3d_wgrad_workspace_bytes(int N, int D, int H, int W, int C, int K, int dtype);
int msseg_dwconv3d_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw, int accumulate, int N, int D,
                         int H, int W, int C, int K, void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Focal modulation (models/backbones/focalnet_3d.py:83-106) on channels-last token volumes of N samples x S voxels x C
 * channels (C a multiple of the 16-byte chunk).  q and the gates are channel ranges of a wider Linear output (voxel strides
 * ldq / ldg; `gates` points at gate 0 of voxel 0); the other activations are dense.
 * spatial_sum: out0[n][c] = scale * sum_v x[n][v][c] * (g ? g[n][v * ldg] : 1); mode 0 also writes out1 = GELU(out0) (if not
 *   null), mode 1 multiplies by gelu'(m_in[n][c]).  Fixed-order sums through `scratch` (msseg_reduce_scratch_bytes()).
 * aggregate_fwd: out = c1 * g0 + c2 * g1 + gm[n][c] * g2.
 * aggregate_bwd: dc1 = da * g0, dc2 = da * g1 + dmv[n][c], dgates[v][0..2] = sum_c da * (c1, c2, gm) and zeros in
 *   dgates[v][3 .. gate_width - 1].
 * mul_fwd: y = q * h.  mul_bwd: dq = dy * h (voxel stride lddq), dh = dy * q.
 * ------------------------------------------------------------------------------------------- */
int msseg_focal_spatial_sum(const void* x, long long ldx, const void* g, long long ldg, const float* m_in, float* out0, float* out1,
                            float scale, int mode, int N, long long S, int C, void* scratch, size_t scratch_bytes, int dtype,
                            msseg_stream_t stream);
int msseg_focal_aggregate_fwd(const void* c1, const void* c2, const void* gates, long long ldg, const float* gm, void* out, int N,
                              long long S, int C, int dtype, msseg_stream_t stream);
int msseg_focal_aggregate_bwd(const void* da, const void* c1, const void* c2, const void* gates, long long ldg, const float* gm,
                              const float* dmv, void* dc1, void* dc2, void* dgates, long long lddg, int gate_width, int N,
                              long long S, int C, int dtype, msseg_stream_t stream);
int msseg_focal_mul_fwd(const void* q, long long ldq, const void* h, void* y, long long rows, int C, int dtype,
                        msseg_stream_t stream);
int msseg_focal_mul_bwd(const void* dy, const void* q, long long ldq, const void* h, void* dq, long long lddq, void* dh,
                        long long rows, int C, int dtype, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SegFormer3D pieces (models/backbones/segformer_backbone.py:51-117, models/segmentors/segformer_head_official.py:65-90).
 * interp_trilinear: F.interpolate(mode='trilinear', align_corners=False) between channels-last volumes
 *   x [N, ID, IH, IW, C] and y [N, OD, OH, OW, C] (C % (16 / sizeof(elem)) == 0); bwd = its adjoint in gather form
 *   (deterministic, one axis per pass, fp32 intermediates in `workspace`): dx from dy; C % 4 == 0 suffices here.
 * kv_attention: o = softmax(q k^T * scale) v per head with few keys (the spatial-reduction attention): q, o [B, N, C],
 *   kv [B, M, 2C] (k = first C channels, v = last C; channel = head * head_dim + c), head_dim in {16, 32, 48, 64};
 *   lse [B, heads, N] fp32 (log-sum-exp of the scaled scores, kept for the backward).  bwd: dq [B, N, C] and
 *   dkv [B, M, 2C] (both fully written); workspace of msseg_kv_attention_bwd_workspace_bytes() holds P, dS and the
 *   per-query-chunk partial sums of dk / dv.
 * scale_channels: y[n, v, c] = x[n, v, c] * scale[n][c] (Dropout3d with a given mask / (1 - p)); dense [N, S, C].
 * ------------------------------------------------------------------------------------------- */
int msseg_interp_trilinear_fwd(const void* x, long long ldx, void* y, long long ldy, int N, int ID, int IH, int IW, int OD,
                               int OH, int OW, int C, int dtype, msseg_stream_t stream);
size_t msseg_interp_trilinear_bwd_workspace_bytes(int N, int ID, int IH, int IW, int OD, int OH, int OW, int C);
int msseg_interp_trilinear_bwd(const void* dy, long long lddy, void* dx, long long lddx, int N, int ID, int IH, int IW, int OD,
                               int OH, int OW, int C, void* workspace, size_t workspace_bytes, int dtype, msseg_stream_t stream);
int msseg_kv_attention_fwd(const void* q, const void* kv, void* o, float* lse, int B, int N, int M, int heads, int head_dim,
                           float scale, int dtype, msseg_stream_t stream);
size_t msseg_kv_attention_bwd_workspace_bytes(int B, int N, int M, int heads, int head_dim);
int msseg_kv_attention_bwd(const void* q, const void* kv, const void* o, const float* lse, const void* dout, void* dq, void* dkv,
                           int B, int N, int M, int heads, int head_dim, float scale, void* workspace, size_t workspace_bytes,
                           int dtype, msseg_stream_t stream);
int msseg_scale_channels(const void* x, const float* scale, void* y, int N, long long S, int C, int dtype, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Normalisation / activation / pooling / layout (HBM-bound, one pass each).
 * ------------------------------------------------------------------------------------------- */
/* Reductions are two-stage and deterministic: blocks write partial rows into `scratch` with plain stores, and a
 * second launch on the same stream adds them in a fixed order.  `scratch` must be 256-byte aligned and at least
 * msseg_reduce_scratch_bytes() long; its first 256 bytes are reserved and neither read nor written, and it needs
 * no initialisation.  Kernels sharing one scratch must be ordered on one stream. */
size_t msseg_reduce_scratch_bytes(void);
/* stats[n][c][0..1] = (sum, sum of squares) over the S voxels of sample n. */
int msseg_channel_stats(const void* x, long long ldx, float* stats, int N, long long S, int C, void* scratch,
                        size_t scratch_bytes, int dtype, msseg_stream_t stream);
/* InstanceNorm3d(eps) [+affine] [+residual] + LeakyReLU(slope) in one pass (slope 1.0 = identity):
 * y = lrelu((x-mean)*rstd*gamma+beta + residual).  nn.InstanceNorm3d + nn.LeakyReLU of UnetResBlock /
 * TwoConv. */
int msseg_instnorm_act_fwd(const void* x, long long ldx, const float* stats, const float* gamma, const float* beta,
                           const void* residual, long long ldr, void* y, long long ldy, int N, long long S, int C,
                           float eps, float slope, int dtype, msseg_stream_t stream);
/* The same fused with the MaxPool3d(2) that follows it in an encoder level (MONAI BasicUNet Down = MaxPool3d(2) -> TwoConv):
 * y as above (no residual) and pooled[n][d/2][h/2][w/2][c] = max over the 2x2x2 cell of y as stored; equals
 * msseg_maxpool2_fwd(y) bit for bit.  D, H, W even; rows 16-byte aligned, C a multiple of 16 / sizeof(element). */
int msseg_instnorm_act_pool_fwd(const void* x, long long ldx, const float* stats, const float* gamma, const float* beta,
                                void* y, long long ldy, void* pooled, long long ldp, int N, int D, int H, int W, int C,
                                float eps, float slope, int dtype, msseg_stream_t stream);
/* Backward of that pair for an encoder level, first pass: da = skip + maxpool2_bwd(y, g) written densely (skip: the
 * decoder's gradient of the level's output, g: gradient of the pooled tensor; y is recomputed from x, arg-max rule as
 * msseg_maxpool2_bwd) and red[n][c] = (sum dz, sum dz*xhat) of da as msseg_instnorm_act_bwd_reduce(y == NULL) gives it,
 * dgamma/dbeta likewise.  Follow with msseg_instnorm_act_bwd_apply(dy = da, red). */
int msseg_instnorm_act_poolbwd_reduce(const void* x, long long ldx, const float* stats, const float* gamma,
                                      const float* beta, const void* skip, long long lds, const void* g, long long ldg,
                                      void* da, long long ldda, float* red, float* dgamma, float* dbeta, int accumulate,
                                      int N, int D, int H, int W, int C, float eps, float slope, void* scratch,
                                      size_t scratch_bytes, int dtype, msseg_stream_t stream);
/* backward, pass 1: red[n][c] = (sum dz, sum dz*xhat), dz = dy * lrelu'(z): the sign of the pre-activation z is taken
 * from the forward output y, or -- y == NULL, layers without residual -- recomputed as x*rstd*gamma + beta - mean*...,
 * which saves one tensor read (gamma/beta = the forward's affine parameters, nullable);
 * optional affine gradients dbeta[c] (+)= sum_n red[n][c][0], dgamma[c] (+)= sum_n red[n][c][1]. */
int msseg_instnorm_act_bwd_reduce(const void* x, long long ldx, const float* stats, const float* gamma,
                                  const float* beta, const void* y, long long ldy,
                                  const void* dy, long long lddy, float* red, float* dgamma, float* dbeta,
                                  int accumulate, int N, long long S, int C, float eps, float slope, void* scratch,
                                  size_t scratch_bytes, int dtype, msseg_stream_t stream);
/* backward, pass 2: dx = rstd*gamma*(dz - red0/S - xhat*red1/S); dres (optional) = dz.  y == NULL as above. */
int msseg_instnorm_act_bwd_apply(const void* x, long long ldx, const float* stats, const float* gamma,
                                 const float* beta, const void* y, long long ldy, const void* dy, long long lddy, const float* red, void* dx,
                                 long long lddx, void* dres, long long lddres, int N, long long S, int C, float eps,
                                 float slope, int dtype, msseg_stream_t stream);
/* msseg_instnorm_act_bwd_apply (y = NULL, no dres) for the unit in front of a <= 4-class 1x1x1 head whose input gradient was
 * not stored (msseg_conv3d_k1_head_bwd_fused with da = NULL): the gradient of the unit's activation is formed again from the
 * class gradient rows dl (16 bytes per voxel, pitch lddl) and the head's weight w[Cout][C], rounded as that kernel stores
 * it; dx has the bits of the plain apply fed with the stored da.  C <= 64 in 16-byte chunks; anything else is an error. */
int msseg_instnorm_act_bwd_apply_head(const void* x, long long ldx, const float* stats, const float* gamma,
                                      const float* beta, const void* dl, long long lddl, const float* w, int Cout,
                                      const float* red, void* dx, long long lddx, int N, long long S, int C, float eps,
                                      float slope, int dtype, msseg_stream_t stream);
/* MaxPool3d(2) forward / backward (first maximum in scan order receives the gradient, as ATen). */
int msseg_maxpool2_fwd(const void* x, long long ldx, void* y, long long ldy, int N, int D, int H, int W, int C,
                       int dtype, msseg_stream_t stream);
int msseg_maxpool2_bwd(const void* x, long long ldx, const void* dy, long long lddy, void* dx, long long lddx,
                       int N, int D, int H, int W, int C, int accumulate, int dtype, msseg_stream_t stream);
/* NCDHW (src_dtype) <-> NDHWC (dst_dtype) */
int msseg_ncdhw_to_ndhwc(const void* src, int src_dtype, void* dst, long long ldd, int dst_dtype, int N, int C,
                         long long S, msseg_stream_t stream);
int msseg_ndhwc_to_ncdhw(const void* src, long long lds, int src_dtype, void* dst, int dst_dtype, int N, int C,
                         long long S, msseg_stream_t stream);
/* out[c] (+)= sum over rows of x[row][c] (bias gradients). */
int msseg_channel_sum(const void* x, long long ldx, float* out, long long rows, int C, int accumulate, void* scratch,
                      size_t scratch_bytes, int dtype, msseg_stream_t stream);
/* y = a + b (elementwise over rows x C with strides) */
int msseg_add(const void* a, long long lda, const void* b, long long ldb, void* y, long long ldy, long long rows,
              int C, int dtype, msseg_stream_t stream);
/* y[n] = a[n] + scale[n] * b[n] over N samples of elems_per_sample dense elements (a NULL: y = scale * b; scale NULL: 1):
 * residual add with the per-sample stochastic-depth factor mask[n] / keep folded in (models/layers/drop_path.py:15-45,
 * swin_nnformer.py:286-287) and the branch gradient of its backward. */
int msseg_axpy_rows(const void* a, const void* b, const float* scale, void* y, int N, long long elems_per_sample, int dtype,
                    msseg_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * Swin transformer pieces (models/backbones/swin_nnformer.py).  Linear layers are msseg_conv3d_k1_* on tokens.
 * ------------------------------------------------------------------------------------------- */
/* Shifted-window attention between the qkv and proj Linears (swin_nnformer.py:128-196 inside :235-289):
 * qkv [B,S,H,W,3C] (channel = which*C + head*hd + e) -> out [B,S,H,W,C].  Window partition, cyclic shift, zero
 * padding to a window multiple (padded tokens carry qkv_bias), the relative-position bias table and the -100 region
 * mask are all applied through addressing; lse [B*nW][heads][ws^3] is saved for the backward.  head_dim in {8,16,32};
 * bf16 with head_dim 16 / 32, C % 8 == 0, ws^3 <= 352 and at most 4095 table rows runs on the MFMA kernels
 * (attention_mfma.hip; the backward only where its LDS image fits), every other case on the fp32-math vector kernels.
 *   bias_ws       the window the bias table was built for: the table has M3 = (2*bias_ws-1)^3 rows of `heads` floats and
 *                 token i of a window takes the relative position of index position decode_{bias_ws}(i).  Default
 *                 bias_ws == ws (0 means ws).  bias_ws > ws is MONAI SwinUNETR's `index[:n, :n]` on a stage whose
 *                 window is clamped to a smaller grid (swin_unetr_official.py:375-385, 477-480).
 *   table_stride  default 0: one table [M3][heads] shared by every sample.  Otherwise one table PER SAMPLE: sample b's
 *                 windows read table + b * table_stride and the backward adds sample b's table gradient to
 *                 dtable + b * table_stride (table_stride >= M3 * heads, in floats).
 *   backward      dqkv is fully written for every token; dtable (nullable = not wanted) is ACCUMULATED (caller
 *                 zero-fills when needed).
 *   workspace     default NULL: the table gradient is summed with LDS float atomics.  With a workspace of at least
 *                 msseg_window_attention_bwd_workspace_bytes(same shape arguments) bytes and a non-NULL dtable, the
 *                 bias-table gradient (swin_nnformer.py:147-155 in reverse) is computed without atomics: dS tiles in
 *                 bf16 -> sum over windows (of one sample at a time with per-sample tables, so the size grows with B)
 *                 -> gather per table entry, deterministic.  The query returns 0 when this shape/dtype has no use for
 *                 a workspace (only the bf16 MFMA backward uses one); a workspace is then ignored. */
int msseg_window_attention_fwd(const void* qkv, const float* qkv_bias, const float* table, void* out, float* lse, int B,
                               int S, int H, int W, int C, int heads, int ws, int shift, int bias_ws, long long table_stride,
                               int dtype, msseg_stream_t stream);
int msseg_window_attention_bwd(const void* qkv, const float* qkv_bias, const float* table, const void* out,
                               const float* lse, const void* dout, void* dqkv, float* dtable, int B, int S, int H, int W,
                               int C, int heads, int ws, int shift, int bias_ws, long long table_stride, int dtype,
                               void* workspace, size_t workspace_bytes, msseg_stream_t stream);
size_t msseg_window_attention_bwd_workspace_bytes(int B, int S, int H, int W, int C, int heads, int ws, int shift,
                                                  int bias_ws, long long table_stride, int dtype);
/* Spacing-conditioned relative position bias (swin_nnformer.py:89-97, :157-166, `--rel_pos_bias_affine`): the per-sample
 * tables T [B][M3][heads] fp32 = table [M3][heads] + lin_b[0] + sum_k lin_w[k] * aff[b][k] * emb [M3][heads][3], for the
 * attention calls above with table_stride = M3 * heads.  aff [B][3] fp32 holds one row per sample.  Every input is read on
 * the device (no host synchronisation). */
int msseg_rel_bias_affine_fold(const float* table, const float* emb, const float* lin_w, const float* lin_b,
                               const float* aff, float* T, int B, int M3, int heads, msseg_stream_t stream);
/* From the per-sample table gradient dT [B][M3][heads]: dtable [M3][heads], demb [M3][heads][3], dlin_w [3], dlin_b [1]
 * (each nullable = not wanted).  Each is overwritten, or added to when its MSSEG_AFFINE_ACC_* bit is set in `flags`.
 * Fixed-order sums, no atomics: bit-identical from run to run.  workspace: msseg_rel_bias_affine_grad_workspace_bytes. */
size_t msseg_rel_bias_affine_grad_workspace_bytes(int M3, int heads);
#define MSSEG_AFFINE_ACC_TABLE 1
#define MSSEG_AFFINE_ACC_EMB 2
#define MSSEG_AFFINE_ACC_LIN_W 4
#define MSSEG_AFFINE_ACC_LIN_B 8
int msseg_rel_bias_affine_grad(const float* dT, const float* emb, const float* lin_w, const float* aff, float* dtable,
                               float* demb, float* dlin_w, float* dlin_b, int B, int M3, int heads, int flags,
                               void* workspace, size_t workspace_bytes, msseg_stream_t stream);
/* LayerNorm over the channel dim of rows x C (nn.LayerNorm, eps 1e-5); mean/rstd [rows] saved for backward. */
int msseg_layernorm_fwd(const void* x, long long ldx, const float* gamma, const float* beta, void* y, long long ldy,
                        float* mean, float* rstd, long long rows, int C, float eps, int dtype, msseg_stream_t stream);
/* input gradient */
int msseg_layernorm_bwd(const void* x, long long ldx, const float* gamma, const float* mean, const float* rstd,
                        const void* dy, long long lddy, void* dx, long long lddx, long long rows, int C, int dtype,
                        msseg_stream_t stream);
/* ... + add: dx = T(layernorm backward) + add, the sum autograd forms when the normalised tensor also feeds a residual branch
 * (x -> LayerNorm and x -> x + f(LayerNorm(x)) in every Swin block, /root/reference/models/backbones/swin_nnformer.py:243-262):
 * one pass instead of the backward + a separate add.  Vector kernel only (C a multiple of the 16-byte chunk, <= 4096). */
int msseg_layernorm_bwd_add(const void* x, long long ldx, const float* gamma, const float* mean, const float* rstd,
                            const void* dy, long long lddy, const void* add, long long ldadd, void* dx, long long lddx,
                            long long rows, int C, int dtype, msseg_stream_t stream);
/* parameter gradients dgamma[c] (+)= sum_rows dy*xhat, dbeta[c] (+)= sum_rows dy (deterministic two-stage reduction) */
int msseg_layernorm_param_grad(const void* x, long long ldx, const float* mean, const float* rstd, const void* dy,
                               long long lddy, float* dgamma, float* dbeta, int accumulate, long long rows, int C,
                               void* scratch, size_t scratch_bytes, int dtype, msseg_stream_t stream);
/* exact (erf) GELU */
int msseg_gelu_fwd(const void* x, void* y, long long n, int dtype, msseg_stream_t stream);
int msseg_gelu_bwd(const void* x, const void* dy, void* dx, long long n, int dtype, msseg_stream_t stream);
/* Linear + GELU of a Swin block's MLP in one pass each way (models/backbones/swin_nnformer.py:24-42 of the reference: fc1,
 * act, fc2; north_star "GELU fusion").  fwd: pre = x W^T + b and act = gelu(pre as stored) from ONE launch (the separate
 * GELU pass re-read pre).  bwd: dpre = (dy W2) * gelu'(pre) -- fc2's input gradient written as fc1's output gradient (the
 * separate pass wrote and re-read the intermediate).  Bit-identical to msseg_conv3d_k1_fwd + msseg_gelu_fwd / _bwd.
 * wp: msseg_pack_weights image (T = 1) of the layer (bwd: of fc2's input-gradient form).  bf16, the register-resident-weight
 * kernel's shapes C -> 4C at C = 48, 96, 192, 384 (msseg_linear_gelu_ok() == 1); callers keep the two-kernel chain otherwise. */
int msseg_linear_gelu_ok(long long NV, int Cin, int Cout, int dtype);
int msseg_linear_gelu_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* pre, long long ldpre, void* act,
                          long long ldact, long long NV, int Cin, int Cout, int dtype, msseg_stream_t stream);
int msseg_linear_gelu_bwd(const void* dy, long long lddy, const void* wp, const void* pre, long long ldpre, void* dpre,
                          long long lddpre, long long NV, int Cin, int Cout, int dtype, msseg_stream_t stream);
/* nn.Linear with the residual add of a Swin block in its epilogue: y = res + (x W^T + b), the sum formed from the bf16-rounded
 * Linear output exactly as Linear followed by an add pass forms it (/root/reference/models/backbones/swin_nnformer.py:243-262:
 * x = shortcut + proj(attn), x = x + mlp(norm2(x))).  msseg_linear_add_ok() == 1 for the shapes the register-resident-weight
 * kernel takes. */
int msseg_linear_add_ok(long long NV, int Cin, int Cout, int dtype);
int msseg_linear_add_fwd(const void* x, long long ldx, const void* wp, const float* bias, const void* res, long long ldres,
                         void* y, long long ldy, long long NV, int Cin, int Cout, int dtype, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dice + cross-entropy loss (MONAI DiceCELoss(to_onehot_y, softmax, squared_pred) as built at
 * run_training.py:103-105, called engine/train.py:62) and the hard Dice metric (engine/train.py:89-111).
 * logits: channels-last [N, S, ld] with ld >= C the voxel stride, or NCDHW when ld == 0; labels: one value
 * per voxel; C <= 16.
 * ------------------------------------------------------------------------------------------- */
/* Four passes for a loss `kind`:
 *  MSSEG_LOSS_DICE_CE: the loss above.
 *  MSSEG_LOSS_TVERSKY (MONAI TverskyLoss(to_onehot_y, softmax, alpha, beta), no squared prediction): slot 1 of partial is
 *    sum p, slot 3 stays 0; loss = mean_{n,c}(1 - (I + snr) / (I + alpha*(P - I) + beta*(T - I) + sdr)); loss[3] =
 *    (tversky, tversky, 0).
 *  MSSEG_LOSS_DICE_FOCAL (MONAI DiceFocalLoss(to_onehot_y, softmax, squared_pred), gamma 2, lambdas 1): slot 3 of partial
 *    is the sum of the SIGMOID focal values of the raw logits (MONAI's FocalLoss does not see the softmax flag), the focal
 *    term their mean over N*C*S elements; loss[3] = (dice + focal, dice, focal).
 *  alpha, beta are read by MSSEG_LOSS_TVERSKY only.  hard[] does not depend on the kind.
 * partials: partial[n][c][0..3] += (sum p*t, sum p^2, sum t, -sum t*log p); hard[n][c][0..2] += (|P&T|, |P|, |T|)
 *    (either pointer may be NULL).  label_dtype: 0 = f32, 1 = bf16, 2 = u8, 3 = i64.
 * finalize: loss[0] = mean_{n,c}(1 - (2I+snr)/(den+sdr)) + CE ; loss[1] = dice term, loss[2] = ce term.
 * fwd: deterministic one-call form of the forward (N <= 8): per-block partial rows in `scratch` (the reduce scratch,
 *    msseg_reduce_scratch_bytes()), added in a fixed order by a one-block second step that also writes partial[N][C][4],
 *    hard[N][C][3] (nullable) and loss[3] = (dice + ce, dice, ce).  No zero-initialised outputs, no atomics: two runs on the
 *    same inputs give the same bits.
 * bwd: dlogits = gscale[0] * dLoss/dlogits (same layout/dtype as logits). */
#define MSSEG_LOSS_DICE_CE 0
#define MSSEG_LOSS_TVERSKY 1
#define MSSEG_LOSS_DICE_FOCAL 2
int msseg_seg_loss_partials(const void* logits, long long ld, int dtype, const void* labels, int label_dtype,
                            float* partial, float* hard, int N, long long S, int C, int kind, msseg_stream_t stream);
int msseg_seg_loss_fwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype, float* partial,
                       float* hard, float* loss, int N, long long S, int C, float smooth_nr, float smooth_dr, int kind,
                       float alpha, float beta, void* scratch, size_t scratch_bytes, msseg_stream_t stream);
int msseg_seg_loss_finalize(const float* partial, float* loss, int N, long long S, int C, float smooth_nr,
                            float smooth_dr, int kind, float alpha, float beta, msseg_stream_t stream);
int msseg_seg_loss_bwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype,
                       const float* partial, const float* gscale, void* dlogits, long long ldd, int N, long long S,
                       int C, float smooth_nr, float smooth_dr, int kind, float alpha, float beta, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Region-based training (nnU-Net's overlapping label regions): channel c of the logits is one SIGMOID output whose
 * target at a voxel with label value `lab` is t = (mask[c] >> lab) & 1 (0 for lab outside 0..31), formed in registers
 * from the label map; no multi-channel label tensor exists.  The masks are read on the host when the call is made and
 * travel in the kernel arguments.  1 <= C <= 16, else MSSEG_EINVAL with nothing launched.
 * ------------------------------------------------------------------------------------------- */
typedef struct { uint32_t mask[16]; } msseg_region_masks;
/* The four passes of msseg_seg_loss_* (same argument lists, layouts, N <= 8 rule of _fwd and scratch) for the sigmoid form
 * of each `kind`.  With p = sigmoid(x), per (n, c): I = sum p*t, T = sum t.
 *  MSSEG_LOSS_DICE_CE: mean_{n,c}(1 - (2I + snr)/(sum p^2 + T + sdr)) + mean_{n,c,s}(max(x,0) - x*t + log1p(exp(-|x|)));
 *    partial[n][c] = (I, sum p^2, T, sum of the BCE values); loss[3] = (dice + bce, dice, bce).
 *  MSSEG_LOSS_TVERSKY: mean_{n,c}(1 - (I + snr)/(I + alpha*(sum p - I) + beta*(T - I) + sdr)); slot 1 is sum p.
 *  MSSEG_LOSS_DICE_FOCAL: the Dice term plus the mean over N*C*S of the sigmoid focal values (gamma 2) against t.
 * hard[n][c] = (|P_c & T_c|, |P_c|, |T_c|) with P_c = (x_c > 0).
 * bwd: dlogits = gscale[0] * dLoss/dlogits; Dice: 1/(N*C) * (-2t/den + (2I + snr)*2p/den^2) * p*(1-p); BCE: (p - t)/(N*C*S);
 *    1 - p is sigmoid(-x), not a subtraction. */
int msseg_region_loss_partials(const void* logits, long long ld, int dtype, const void* labels, int label_dtype,
                               float* partial, float* hard, int N, long long S, int C, int kind,
                               const msseg_region_masks* masks, msseg_stream_t stream);
int msseg_region_loss_fwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype, float* partial,
                          float* hard, float* loss, int N, long long S, int C, float smooth_nr, float smooth_dr, int kind,
                          float alpha, float beta, const msseg_region_masks* masks, void* scratch, size_t scratch_bytes,
                          msseg_stream_t stream);
int msseg_region_loss_finalize(const float* partial, float* loss, int N, long long S, int C, float smooth_nr,
                               float smooth_dr, int kind, float alpha, float beta, msseg_stream_t stream);
int msseg_region_loss_bwd(const void* logits, long long ld, int dtype, const void* labels, int label_dtype,
                          const float* partial, const float* gscale, void* dlogits, long long ldd, int N, long long S,
                          int C, float smooth_nr, float smooth_dr, int kind, float alpha, float beta,
                          const msseg_region_masks* masks, msseg_stream_t stream);
/* logits fp32 [C][V] -> label map: bits = sum_c (logits[c][v] > 0) << c (NaN does not fire); out[v] = 0, then for c = 0..C-1
 * in order: if bit c is set, out[v] = values[c] (later regions paint over earlier ones, nnU-Net's regions_class_order).
 * values: C bytes on the host.  bits: nullable, the fired-region set per voxel. */
int msseg_region_decode_u8(const float* logits, int C, long long V, const uint8_t* values, uint8_t* out, uint16_t* bits,
                           msseg_stream_t stream);
/* counts[c][0..2] = (|P_c & T_c|, |P_c|, |T_c|) of two uint8 label maps, both taken through the masks (a value above 31 is in
 * no region).  Per-block integer counts into `scratch` (the reduce scratch), added in a fixed order in 64-bit integers by a
 * second step; exact up to 2^24 per count (the float output). */
int msseg_region_counts_u8(const uint8_t* pred, const uint8_t* label, long long V, int C, const msseg_region_masks* masks,
                           float* counts, void* scratch, size_t scratch_bytes, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser: fused AdamW over one flat fp32 buffer (torch.optim.AdamW(betas=(0.9,0.95), eps=1e-6) of
 * run_training.py:92-93; decay applies where decay_mask[i] != 0 -- timm add_weight_decay semantics).
 * grad_scale[0] multiplies the gradient first (clip coefficient / loss-scale inverse).
 * ------------------------------------------------------------------------------------------- */
int msseg_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                     long long n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                     const float* grad_scale, const float* dev_hyper /* nullable: device [lr, step] overriding the
                     host values, so a captured hipGraph can be replayed while the schedule advances */,
                     msseg_stream_t stream);
/* out[0] = sum of squares of x[0..n), added in a fixed order (bit-identical from run to run): per-block sums into
   partials[0..n_partials) -- a buffer of the caller, at most n_partials blocks are launched (4096 is plenty) -- then one
   block adds them and overwrites out[0]. */
int msseg_sumsq(const float* x, long long n, float* out, float* partials, int n_partials, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sliding-window inference (engine/utils.py:120-151): gather windows, weighted blend, normalise.
 * ------------------------------------------------------------------------------------------- */
int msseg_sw_normalize(float* out, const float* cnt, int C, long long V, msseg_stream_t stream);
/* One launch per window batch (the reference's loop body engine/utils.py:120-148 for `sw_batch_size` windows at
 * once).  imp: fp32 [roi] importance map; cnt has one channel.
 * table: device int32 [nwin][4] = (sample b, z0, y0, x0); b < 0 = unused slot.
 * gather: win[j] = window j of vol[b] (fp32 [B][C][VD][VH][VW], sample stride vol_bstride elements), `cval` outside;
 *         win layout NCDHW [nwin][C][roi] when ldw == 0, channels-last [nwin][roi][ldw] otherwise.
 * blend : out[b][c][vol] += imp * win[j][c], cnt[b][vol] += imp for every window of the table, each output voxel
 *         accumulated in table order with the reference's roundings (bit-identical to blending the nwin windows one
 *         after the other); windows of one batch may overlap.  nwin <= 256, C <= 16. */
/* A mirror mask per table row (mirror test-time augmentation: a (window, mask) pair is one more row).  flips: device
 * int32 [nwin], bit 0 / 1 / 2 set = row j is mirrored along D / H / W; null = no row is mirrored, which is exactly the
 * above.  With f(r) = R - 1 - r on a mirrored axis of extent R and f(r) = r otherwise:
 * gather: win[j][rz][ry][rx] = vol[b][z0 + fz(rz)][y0 + fy(ry)][x0 + fx(rx)], `cval` outside -- the window as above,
 *         flipped along the mirrored axes.
 * blend : out[b][c][z0+dz][y0+dy][x0+dx] += imp[dz][dy][dx] * win[j][c][fz(dz)][fy(dy)][fx(dx)], cnt += imp[dz][dy][dx]:
 *         the logits are un-mirrored on the way in, the weight is NOT mirrored (it is indexed in volume orientation;
 *         the Gaussian map of an even extent peaks at R / 2 and is not symmetric).  Order and roundings as above;
 *         rows of one start under several masks overlap completely.  RD, RH, RW are independent, even or odd. */
int msseg_sw_gather_batch(const float* vol, long long vol_bstride, void* win, long long ldw, int dtype, const int* table,
                          const int* flips, int nwin, int C, int VD, int VH, int VW, int RD, int RH, int RW, float cval,
                          msseg_stream_t stream);
int msseg_sw_blend_batch(const void* win, long long ldw, int dtype, const float* imp, float* out, long long out_bstride,
                         float* cnt, long long cnt_bstride, const int* table, const int* flips, int nwin, int C, int VD,
                         int VH, int VW, int RD, int RH, int RW, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Layout passes of the vendored MONAI Swin-UNETR encoder (csrc/layout.hip; /root/reference/models/segmentors/
 * swin_unetr_official.py:244-270,699-712), channels-last volumes, 16-byte channel chunks (C % 8 == 0 bf16, % 4 fp32).
 * msseg_box_copy: dst[n, d, h, w, :C] = src[n, d, h, w, :C] inside the common box, zero elsewhere in dst -- F.pad with zeros at
 *   the high end when dst is larger, the crop x[:, :d, :h, :w] when it is smaller (each is the other's adjoint).
 * msseg_merge_gather_fwd: out[n, i, j, k, s*C + c] = x[n, 2i + a_s, 2j + b_s, 2k + c_s, c] (zero beyond the grid) for eight
 *   sub-grids; `subs` holds 3 bits per slot s at bits 3s..3s+2 (bit 0: offset along D, bit 1: H, bit 2: W); duplicates allowed
 *   (PatchMerging's x5 == x2, x6 == x3).  out: [N, ceil(D/2), ceil(H/2), ceil(W/2), 8C].  _bwd: the adjoint (per fine voxel the
 *   sum, in slot order, of the slots whose offset equals the voxel's parity; deterministic).
 * ------------------------------------------------------------------------------------------- */
int msseg_box_copy(const void* src, long long lds, int SD, int SH, int SW, void* dst, long long ldd, int DD, int DH, int DW,
                   int N, int C, int dtype, msseg_stream_t stream);
int msseg_merge_gather_fwd(const void* x, long long ldx, int D, int H, int W, void* out, long long ldo, int N, int C,
                           unsigned subs, int dtype, msseg_stream_t stream);
int msseg_merge_gather_bwd(const void* dy, long long lddy, void* dx, long long lddx, int N, int D, int H, int W, int C,
                           unsigned subs, int dtype, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Post-inference (the step right after the path).
 * argmax_u8: out[v] = first arg max over c of logits[c][v] (NCDHW fp32, one sample) -- engine/test.py:140-141
 *            (softmax is monotonic, so it is skipped).
 * resample_nearest_u8: scipy.ndimage.zoom(order=0, prefilter=False) of a uint8 label map to (TD, TH, TW) --
 *            utils/misc.py:420-425; coordinates in double exactly as scipy forms them.
 * majority_vote_u8: labels [F][V] -> out[V]; votes[c] = #folds with label c for c >= 1, votes[0] = 1, first maximum --
 *            majority_vote.py:23-37.
 * ------------------------------------------------------------------------------------------- */
int msseg_argmax_u8(const float* logits, int C, long long V, uint8_t* out, msseg_stream_t stream);
int msseg_resample_nearest_u8(const uint8_t* src, int SD, int SH, int SW, uint8_t* dst, int TD, int TH, int TW,
                              msseg_stream_t stream);
int msseg_majority_vote_u8(const uint8_t* labels, int F, long long V, int C, uint8_t* out, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Hausdorff-95 of eval_model (engine/test.py:31,48-51,64: MONAI HausdorffDistanceMetric(include_background=True,
 * percentile=95, reduction="mean", get_not_nans=True)).  Exact integer work on uint8 label maps [D][H][W]:
 * hd_edges: surface voxels (6-neighbour erosion XOR, outside = background) of both maps for all classes: edge maps hold
 *            the class on surface voxels and 0xFF elsewhere; stats[c][8] = {min z, y, x, max z, y, x (inclusive) of class
 *            c's surface voxels of BOTH maps, #surface voxels of pred, of gt}.
 * hd_directed_hist: hist[d2] = number of class-`cls` surface voxels of `edges_tgt` whose squared Euclidean distance (voxel
 *            units) to the nearest class-`cls` surface voxel of `edges_src` is d2, searched inside box6 = {z0, y0, x0, z1,
 *            y1, x1} (half-open; must contain both surfaces: hd_edges' box); bin nbins-1 counts voxels with no source voxel.
 *            nbins >= (bz-1)^2 + (by-1)^2 + (bx-1)^2 + 2.  The caller takes the percentile's order statistics from the
 *            histogram and the square roots in double (scipy.ndimage.distance_transform_edt's values).
 * ------------------------------------------------------------------------------------------- */
int msseg_hd_edges(const uint8_t* pred, const uint8_t* gt, int D, int H, int W, int C, uint8_t* edges_pred,
                   uint8_t* edges_gt, int* stats, msseg_stream_t stream);
size_t msseg_hd_directed_workspace_bytes(int bz, int by, int bx);
int msseg_hd_directed_hist(const uint8_t* edges_src, const uint8_t* edges_tgt, int cls, int D, int H, int W,
                           const int* box6, void* workspace, size_t workspace_bytes, int* hist, int nbins,
                           msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Surface distances in millimetres (metrics.surface_metrics: HD percentile, average symmetric surface distance, normalised
 * surface Dice of one pair of label maps on an anisotropic grid).  Edge maps, box and surface sizes are hd_edges'.
 * sd_directed_mm: d2map[bz][by][bx] (box-local, dense, double) = the exact squared Euclidean distance in physical units from
 *            every class-`cls` surface voxel of `edges_tgt` to the nearest class-`cls` surface voxel of `edges_src` inside
 *            box6 (as hd_directed_hist's); -1 at every other voxel of the box; +inf at the surface voxels when `edges_src`
 *            has no class-`cls` voxel in the box.  spacing3 = {sz, sy, sx}: HOST doubles, one per tensor axis, finite and
 *            positive.  A term is (s k)^2 with k the integer voxel offset, the sum is (x term + y term) + z term, every
 *            operation rounds once (no contraction).  Workspace: 10 bytes per box voxel (sd_directed_workspace_bytes).
 * sd_summary: reduces such a map of n entries on the device into out16 (DEVICE, 16 slots of 8 bytes):
 *            [0] number of entries >= 0 (surface voxels), [1] number of +inf entries, [2] sum of sqrt(d2) over the finite
 *            entries (double; fixed-shape two-level reduction: same bits on every run), [3 + j] number of entries with
 *            sqrt(d2) <= tolerances[j] (compared in double on the square root), [11 + r] the order statistic of d2 at the
 *            zero-based rank ranks[r] (double; NaN when the rank is past the last entry), [15] 0.  tolerances (ntol <= 8) and
 *            ranks (nrank <= 4, >= 0) are HOST arrays.  Order statistics by radix select over the doubles' bit patterns;
 *            counts by integer atomics.  scratch: DEVICE, 8-byte aligned, sd_summary_scratch_bytes(), no initialisation.
 * ------------------------------------------------------------------------------------------- */
size_t msseg_sd_directed_workspace_bytes(int bz, int by, int bx);
int msseg_sd_directed_mm(const uint8_t* edges_src, const uint8_t* edges_tgt, int cls, int D, int H, int W, const int* box6,
                         const double* spacing3, void* workspace, size_t workspace_bytes, double* d2map,
                         msseg_stream_t stream);
size_t msseg_sd_summary_scratch_bytes(void);
int msseg_sd_summary(const double* d2map, long long n, const double* tolerances, int ntol, const long long* ranks, int nrank,
                     void* scratch, size_t scratch_bytes, void* out16, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Keep the largest connected component per class (csrc/components.hip): MONAI KeepLargestConnectedComponent(
 * applied_labels=1..n_classes-1, is_onehot=False, independent=True) on a uint8 label map [D][H][W].
 * For each class c in 1..n_classes-1 independently: the connected components of lab == c (connectivity 6: face
 * neighbours; 26: face, edge and corner neighbours; outside the volume counts as background); the component with the most
 * voxels is kept -- among equal sizes the one whose first voxel in flat [D][H][W] order comes first, scipy's numbering with
 * argmax(bincount) -- and every other voxel of class c becomes 0.  Class 0 and values >= n_classes (an ignore label such
 * as 255) are copied unchanged and join no component.
 * work: 2 * D*H*W int32 (labels, counters; contents undefined afterwards).  stats[c][4] = {number of components, voxels
 * kept, flat index of the kept component's first voxel (-1: class absent), voxels removed}; row 0 is {0, 0, -1, 0}; 8-byte
 * aligned.  out == lab (in place) is allowed.  MSSEG_EINVAL for a connectivity other than 6 / 26, n_classes outside 2..64,
 * null pointers, D*H*W >= 2^31.  Lock-free integer atomics only: bit-identical from run to run.  No host synchronisation,
 * no device-to-host copy: the caller reads `stats`.
 * ------------------------------------------------------------------------------------------- */
int msseg_keep_largest_u8(const uint8_t* lab, int D, int H, int W, int n_classes, int connectivity, int32_t* work,
                          int32_t* stats, uint8_t* out, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Post-processing of a uint8 label map [D][H][W] (csrc/components.hip): up to three steps, always in this order, each
 * optional.  Semantics pinned to scipy (tests/postproc_ref.py); parity with MONAI unpinned.
 *  1 remove small components (MONAI RemoveSmallObjects, nnU-Net): min_size = N; 0 and 1 switch the step off.  Each class c
 *    in 1..n_classes-1 is labelled independently with `connectivity` (6 or 26); every component with fewer than N voxels
 *    becomes 0.
 *  2 keep the largest component per class (keep_largest != 0): msseg_keep_largest_u8's rule on what step 1 left -- the same
 *    labelling and sizes serve both; a class whose largest component is below N ends up empty.
 *  3 fill holes (fill_holes != 0; MONAI FillHoles): for c = 1, 2, .., n_classes-1 in this order, each on the map the class
 *    before left, every voxel that cannot be reached from outside the volume through voxels != c becomes c
 *    (out[scipy.ndimage.binary_fill_holes(out == c, structure)] = c).  `hole_connectivity` (6 or 26) is the neighbourhood of
 *    the leak path: a diagonal gap in a wall leaks at 26 and not at 6.  Enclosed voxels of other classes and of values >=
 *    n_classes are overwritten; a region that touches one of the six volume faces is no hole.  One labelling of the
 *    complement per foreground class.
 * In steps 1 and 2 class 0 and values >= n_classes are copied and join nothing.  With all three steps off the call is a copy.
 * work: 2 * D*H*W int32 (contents undefined afterwards).  stats[c][6], 8-byte aligned, row 0 all zero = {components before
 * any step (-1 when neither step 1 nor step 2 is on: the classes are then not labelled), components removed as small, voxels
 * removed as small, voxels removed by keep-largest, voxels turned into c by its fill step, voxels of class c in the final
 * map}.  out == lab (in place) is allowed.  MSSEG_EINVAL for a connectivity or hole connectivity other than 6 / 26 (checked
 * whether or not the step is on), n_classes outside 2..64, a negative min_size, null or misaligned pointers, D*H*W >= 2^31.
 * Lock-free integer atomics only: bit-identical from run to run.  No host synchronisation: the caller reads `stats`.
 * ------------------------------------------------------------------------------------------- */
int msseg_postprocess_u8(const uint8_t* lab, int D, int H, int W, int n_classes, int min_size, int keep_largest,
                         int connectivity, int fill_holes, int hole_connectivity, int32_t* work, int32_t* stats,
                         uint8_t* out, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Device-side training crop + augmentation (the step right before the path): one gather launch per
 * batch of patches from a volume cached in HBM.  Replaces RandCropByPosNegLabeld + RandFlipd x3 + RandRotate90d +
 * RandShiftIntensityd + RandScaleIntensityd (data/dataset_builder.py:108-193); the random draws arrive in `table`.
 * img: fp32 [C][VD][VH][VW]; lab: uint8 [VD][VH][VW] or NULL; out_img: [npatch][C][R][R][R] (out_dtype), out_lab: fp32
 * [npatch][1][R][R][R].  Row: crop start (z0, y0, x0), flips bit0/1/2 = axis d/h/w, rotk = quarter turns in the (d, h)
 * plane (np.rot90 sense), image value = (v + shift) * scale.
 * ------------------------------------------------------------------------------------------- */
typedef struct msseg_aug_row { int32_t z0, y0, x0, flips, rotk, pad0; float shift, scale; } msseg_aug_row;
int msseg_aug_crop_batch(const float* img, const uint8_t* lab, int C, int VD, int VH, int VW, const void* table,
                         int npatch, void* out_img, int out_dtype, float* out_lab, int R, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dataset path (csrc/dataprep.hip): one-off preprocessing of a loaded volume on the device and the per-step patch gather
 * over many cached volumes.  Volumes are NCDHW single samples of arbitrary D x H x W.  MONAI parity unpinned: the
 * semantics are those of the numpy / scipy restatement in tests/dataprep_ref.py.
 * intensity_prep: src fp32 (src_dtype 0) or int16 (1) [C][D][H][W] -> dst fp32.  mode 0: copy; 1: ScaleIntensityRange(a_min,
 *            a_min + a_range, 0, 1, clip=True); 2: the same after cbrt (a_min / a_range are those of the cube roots of
 *            the bounds, data/transforms.py:45-75); then (v - subtrahend) / divisor when `normalize`.  One fp32 rounding per
 *            numpy operation.  box6 (device, 6 ints) = {min z, y, x, max z, y, x (inclusive)} over voxels where any channel
 *            is > 0 after scaling and before normalisation (CropForegroundd(source_key="image")); {D, H, W, -1, -1, -1}
 *            when there is none.
 * resample_spacing: Spacingd.  Source coordinate = destination index * r (r = new / old spacing per axis, double).  Image
 *            (fp32, is_label 0): trilinear, border clamped; label (uint8, is_label 1): nearest, floor(c + 0.5).
 * crop_pad_copy: dst[c][pad_before + i] = src[c][box start + i] for i inside box6 = {z0, y0, x0, z1, y1, x1} (half-open,
 *            HOST ints, as pad_before3), the pad value elsewhere; elem_bytes 4 (fp32) or 1 (uint8).
 * slab_counts: counts[z] = {#(lab > 0), #(lab == 0 && image_ok(img0))} per z-slice, int32 [D][2] on the device.  The image
 *            side of a background candidate is chosen by bg_rule: 0 = img0 > threshold, 1 = img0 != threshold: the non-zero
 *            mask of a z-scored cache (msseg_zscore_apply), whose in-mask values have either sign.
 * pick_voxels: rows[i] = msseg_pick_row; mode 1 / 0: the rank-th foreground / background voxel (flat order) of slice z of
 *            volume vol; mode 2: rank IS the in-slice flat index.  out[i][8] = {centre z, y, x (MONAI correct_crop_centers
 *            clamp for the cubic roi R), crop start z, y, x, z, in-slice flat index of the voxel (-1: rank beyond the count)}.
 * aug_crop_multi: msseg_aug_crop_batch over many volumes: row i reads volume rows[i].vol at the crop start picks[i][3..5]
 *            (clamped into the volume) with the row's flips / rotk / shift / scale; out_img [npatch][C][R][R][R] fp32 or bf16,
 *            out_lab fp32 [npatch][1][R][R][R].  One launch per batch.  Precondition (the tables live on the device, so the
 *            entry point cannot check it; DeviceDatasetLoader does on the host): every rows[i].vol is in [0, nvol), that
 *            volume has C channels and is at least R long on every axis.  A row that breaks it reads nothing and yields
 *            an all-zero patch; the call still returns MSSEG_OK.
 * aug_crop_affine: aug_crop_multi that samples the cached VOLUME under a row-major 3x3 matrix M per patch (mats: npatch x 9
 *            doubles on the device) instead of copying the crop: free rotation and zoom about the patch's geometric centre,
 *            still one launch per batch.  Output voxel -> patch index p (rotk and flips undone as in aug_crop_multi, crop
 *            start clamped the same way); source coordinate per axis a, in double with one rounding per operation:
 *            c[a] = (start[a] + h) + ((M[a][0] d[0] + M[a][1] d[1]) + M[a][2] d[2]), h = (R - 1) / 2.0, d = p - h.  Image:
 *            trilinear over the 8 taps at floor(c), fp32 lerps a + f * (b - a) along x, then y, then z with f = (float)(c -
 *            floor(c)); a tap with any index outside the volume reads pad_value (scipy mode="grid-constant"); then
 *            (v + shift) * scale.  Label: the voxel floor(c + 0.5), 0 outside the volume or without a label pointer.  With
 *            M = I the output is bit for bit that of aug_crop_multi.  Invalid rows as in aug_crop_multi.
 * ------------------------------------------------------------------------------------------- */
typedef struct msseg_volume_desc { const float* img; const uint8_t* lab; int32_t C, D, H, W; } msseg_volume_desc;
typedef struct msseg_pick_row { int32_t vol, mode, z, rank, flips, rotk; float shift, scale; } msseg_pick_row;
int msseg_intensity_prep(const void* src, int src_dtype, int C, int D, int H, int W, int mode, float a_min, float a_range,
                         int normalize, float subtrahend, float divisor, float* dst, int* box6, msseg_stream_t stream);
int msseg_resample_spacing(const void* src, int is_label, int C, int SD, int SH, int SW, void* dst, int TD, int TH, int TW,
                           double rz, double ry, double rx, msseg_stream_t stream);
int msseg_crop_pad_copy(const void* src, int elem_bytes, int C, int SD, int SH, int SW, const int* box6, void* dst, int TD,
                        int TH, int TW, const int* pad_before3, float pad_f32, int pad_u8, msseg_stream_t stream);
int msseg_slab_counts(const float* img0, const uint8_t* lab, int D, int H, int W, float threshold, int bg_rule, int* counts,
                      msseg_stream_t stream);
int msseg_pick_voxels(const void* volumes, int nvol, const void* rows, int nrows, int R, float threshold, int bg_rule, int* out,
                      msseg_stream_t stream);
int msseg_aug_crop_multi(const void* volumes, int nvol, const void* rows, const int* picks, int npatch, int C, void* out_img,
                         int out_dtype, float* out_lab, int R, msseg_stream_t stream);
int msseg_aug_crop_affine(const void* volumes, int nvol, const void* rows, const int* picks, const double* mats, int npatch,
                          int C, void* out_img, int out_dtype, float* out_lab, int R, float pad_value, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Class-ratio crop centres (csrc/class_crop.hip; the reference's RandCropByLabelClassesd, --t_rand_crop_class_ratios /
 * --t_rand_crop_center_dilation here).  Semantics: tests/class_crop_ref.py.  With image_ok(v) = v > threshold (bg_rule 0)
 * or v != threshold (bg_rule 1) as in slab_counts, voxel v is a candidate of class c < K iff image_ok(img0(v)) and a
 * voxel u with lab(u) == c exists with |u - v|_1 <= N; N = 0: lab(v) == c.  Label values >= K belong to no class.
 * A class pick is a msseg_pick_row with mode = MSSEG_PICK_CLASS0 + c; the gather kernels never read mode.
 * class_candidate_mask: N > 0, once per cached volume.  mask (device, uint16 [D][H][W]) gets bit c = that predicate for every
 *            class c of class_bits (bits 0..15), 0 for the others.  0 <= N <= 254.  scratch: D * H * W bytes on the device,
 *            reused by the classes.  Per class three capped chamfer sweeps of the L1 distance to the class (forward and
 *            backward along x, then y, then z, capped at N + 1 so that it fits a byte); equal to scipy's
 *            binary_dilation(lab == c, iterations=N) with the default structure.
 * class_slab_counts: counts[z][c], int32 [D][K] on the device, 1 <= K <= 16: the candidates of class c in slice z, read from
 *            mask when it is not NULL (img0 and lab are then unused and may be NULL), from (img0, lab) with N = 0 otherwise.
 * class_pick_voxels: pick_voxels whose rows may also carry mode 16 + c: the rank-th candidate of class c (flat order)
 *            of slice z of volume vol, read from masks[vol] when masks (NULL, or a device array of nvol mask pointers) and
 *            that entry are not NULL, from the volume's label with N = 0 otherwise.  Rows of mode 0, 1, 2 and the output
 *            row are exactly those of pick_voxels; any other mode reports -1 as a rank beyond the count does.
 * ------------------------------------------------------------------------------------------- */
#define MSSEG_PICK_CLASS0 16
int msseg_class_candidate_mask(const float* img0, const uint8_t* lab, int D, int H, int W, float threshold, int bg_rule,
                               unsigned class_bits, int N, uint8_t* scratch, uint16_t* mask, msseg_stream_t stream);
int msseg_class_slab_counts(const float* img0, const uint8_t* lab, const uint16_t* mask, int D, int H, int W, int K,
                            float threshold, int bg_rule, int* counts, msseg_stream_t stream);
int msseg_class_pick_voxels(const void* volumes, const void* masks, int nvol, const void* rows, int nrows, int R,
                            float threshold, int bg_rule, int* out, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-volume z-score over the non-zero voxels (csrc/volume_stats.hip): the last step of the dataset path's preprocessing
 * for MR data (--t_zscore / --t_zscore_clip; nnU-Net's ZScoreNormalization with use_mask_for_norm, per channel of each
 * volume; no reference counterpart: the reference normalises per cropped patch).  x: fp32 [C][V], 16-byte aligned,
 * 1 <= C <= 1024, 1 <= V < 2^32.  The mask of a channel is x != 0 (-0.0 is outside it), n its size.  Semantics:
 * tests/zscore_ref.py.  Everything is enqueued on the stream; nothing is read back.  scratch:
 * msseg_volume_stats_scratch_bytes(C) bytes, 8-byte aligned, shared by select_f32 and masked_moments (calls on one stream).
 * select_f32: exact order statistics of the masked values of every channel (radix select, 4 passes over x).  Either
 *            `ranks` (HOST, 1..4 zero-based ranks, percentages NULL) or `percentages` (HOST, 1..2 values q in [0, 100], ranks
 *            NULL): then the ranks are k = floor(h) and min(k + 1, n - 1) per percentage, h = q / 100 * (n - 1), formed on the
 *            device from n.  out8 (device) [C][8] doubles = {n, the up to 4 order statistics in the order asked for (k, k + 1
 *            of the first percentage, then of the second; NaN: rank >= n or not asked for), P of the first and of the second
 *            percentage, 0}; P = x_(k) + (h - k) (x_(k+1) - x_(k)) in double, rounded once to fp32 (numpy's "linear"
 *            percentile); a slot whose percentile is not formed (ranks given, no second percentage, n == 0) holds -inf
 *            (first) or +inf (second), i.e. no clip on that side.
 * masked_moments: stats6 (device) [C][6] doubles = {n, lo, hi, mean, std, number of non-finite masked values}.  lo / hi:
 *            the clip bounds of channel c read from bounds[c * bound_stride + 0 / 1] (device doubles, rounded to fp32; e.g.
 *            out8 + 5 with stride 8), -inf / +inf when bounds is NULL.  With y = min(max(x, lo), hi) on the mask:
 *            mean = sum y / n and std = sqrt(sum (y - mean)^2 / n) (population, second pass over the deviations from the
 *            double mean), both in double; a std that is 0 as fp32 -> 1; n == 0 -> mean 0, std 1.  2 passes over x.
 *            Per-block partial rows in double summed in a fixed order: bit-identical from run to run.
 * zscore_apply: in place, x = (min(max(x, lo), hi) - mean) / std on the mask with lo, hi, mean, std of stats6 each rounded
 *            once to fp32, one fp32 rounding per operation; voxels outside the mask keep their bits.
 * ------------------------------------------------------------------------------------------- */
size_t msseg_volume_stats_scratch_bytes(int C);
int msseg_select_f32(const float* x, int C, long long V, const long long* ranks, int nrank, const double* percentages, int npct,
                     void* scratch, size_t scratch_bytes, double* out8, msseg_stream_t stream);
int msseg_masked_moments(const float* x, int C, long long V, const double* bounds, long long bound_stride, void* scratch,
                         size_t scratch_bytes, double* stats6, msseg_stream_t stream);
int msseg_zscore_apply(float* x, int C, long long V, const double* stats6, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Intensity augmentation of a gathered batch (csrc/intensity_aug.hip; no reference counterpart: the reference has no
 * noise / blur / contrast / gamma transform; the recipe and its order are nnU-Net's).  x: fp32 [N][C][D][H][W], the gather's
 * output; out: the same shape in out_dtype (MSSEG_F32 / MSSEG_BF16), out != x; one msseg_intensity_row per (patch, channel),
 * row n * C + c.  The table is passed twice: rows_dev is read by the kernels, rows_host (the same N * C rows in host memory,
 * read before the call returns) is what the entry point validates and plans its launches from.  Stages, in this order, on
 * each row whose bit is set (semantics: tests/intensity_aug_ref.py, float64):
 *   NOISE      x += noise_std * z(noise_key, i), i = flat voxel index inside the (patch, channel).  Philox4x32-10, counter
 *              {i lo, i hi, 0, 0}, key {noise_key lo, hi}; u1, u2 = ((word0, word1 >> 8) + 0.5) * 2^-24 in fp32;
 *              z = sqrt(-2 ln u1) cos(2 pi u2).
 *   BLUR       scipy.ndimage.gaussian_filter(x, blur_sigma, mode="reflect", truncate=4) over D, H, W: radius
 *              int(4 sigma + 0.5), weights exp(-k^2 / (2 sigma^2)) normalised.
 *   CONTRAST   x = clip((x - m) * contrast + m, lo, hi); m, lo, hi = mean, min, max of the row at this point.
 *   GAMMA_INV  the GAMMA formula with gamma_inv on -x, negated back.
 *   GAMMA      m, s = mean, population std; lo = min, R = max - lo; y = ((x - lo) / (R + 1e-7))^gamma * R + lo;
 *              x = (y - mean(y)) / (std(y) + 1e-8) * s + m.
 * A row with no bit set is copied (converted).  Deterministic: per-block partials combined in a fixed order, no
 * floating-point atomics.  MSSEG_EINVAL, with nothing launched, for a patch dimension outside 8..4096, N * C > 65535, a
 * blur sigma outside (0, 2] (radius above 8), a negative or non-finite noise std, a gamma <= 0, unknown mask bits, a bad
 * dtype.  workspace: msseg_intensity_aug_workspace_bytes(...) bytes, 16-byte aligned; needed only when a contrast or gamma
 * bit is set (MSSEG_EWORKSPACE otherwise).  Launches: 1 (noise / blur / copy) + 1 if any row has CONTRAST + 2 per gamma kind
 * present.  msseg_intensity_noise_bits: the four Philox words of counters first .. first + n - 1 under the key {key_lo, key_hi}, uint32 [n][4]
 * (test aid for the generator's integer stage).
 * ------------------------------------------------------------------------------------------- */
#define MSSEG_INTENSITY_NOISE 1u
#define MSSEG_INTENSITY_BLUR 2u
#define MSSEG_INTENSITY_CONTRAST 4u
#define MSSEG_INTENSITY_GAMMA_INV 8u
#define MSSEG_INTENSITY_GAMMA 16u
/* 32 bytes; offsets: mask 0, noise_std 4, noise_key 8, blur_sigma 16, contrast 20, gamma_inv 24, gamma 28 */
typedef struct msseg_intensity_row {
    uint32_t mask; float noise_std; uint64_t noise_key; float blur_sigma, contrast, gamma_inv, gamma;
} msseg_intensity_row;
size_t msseg_intensity_aug_workspace_bytes(int N, int C, int D, int H, int W);
int msseg_intensity_aug(const float* x, const msseg_intensity_row* rows_host, const void* rows_dev, int N, int C, int D, int H,
                        int W, void* out, int out_dtype, void* workspace, size_t workspace_bytes, msseg_stream_t stream);
int msseg_intensity_noise_bits(unsigned key_lo, unsigned key_hi, long long first, long long n, uint32_t* out, msseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Prediction -> the grid of the file it came from (csrc/restore.hip): the inverse of the dataset path's chain
 * Orientationd(RAS) -> Spacingd -> CropForegroundd -> SpatialPadd in ONE launch (no reference counterpart: the reference's
 * test_model zooms the cropped map to the uncropped size).  desc is a HOST pointer to one msseg_restore_desc, read before
 * the call returns; it travels to the kernel as an argument.  src: uint8 [model] (src_is_logits 0, C ignored) or fp32
 * [C][model] (src_is_logits 1); dst: uint8 [native], C-contiguous in the file array's order.
 * Per native voxel n and oriented axis k, in double with one rounding per operation:
 *   o = n[perm[k]], or native[perm[k]] - 1 - o when flip[k];  s = min(o * scale[k], grid[k] - 1)  (the spacing step rounds
 *   the length, the last native voxels may land up to half a voxel beyond the grid);  m[k] = s + offset[k];
 *   q[k] = floor(m[k] + 0.5).  Any q[k] outside [0, model[k]): the voxel was cropped away as air, dst = 0 in both modes.
 * Nearest (labels): dst = src[q].
 * Linear (logits): taps i0 = floor(m[k]) and i0 + 1, each clamped into [0, model[k] - 1], f[k] = (float)(m[k] - i0); per
 *   channel fp32 lerps a + f * (b - a) along model axis 2, then 1, then 0 (msseg_resample_spacing's order); dst = the first
 *   channel with the strictly greatest value (msseg_argmax_u8's rule).  [C][native] is never formed: the call reads src
 *   through the cache and writes one byte per native voxel.
 * MSSEG_EINVAL, with nothing launched: perm is not a permutation, a dimension < 1, a scale that is not finite or not > 0,
 * C outside 1..255 with logits, native axis 0 or 1 longer than 65535.
 * ------------------------------------------------------------------------------------------- */
typedef struct msseg_restore_desc {
    int32_t native[3];  /* file array shape */
    int32_t perm[3];    /* oriented axis k is native axis perm[k] */
    int32_t flip[3];    /* oriented axis k runs backwards */
    int32_t grid[3];    /* shape after the spacing resample, before crop + pad */
    int32_t offset[3];  /* pad_before[k] - box_lo[k] */
    int32_t model[3];   /* shape of src's spatial grid */
    double  scale[3];   /* old / new spacing per oriented axis; 1.0 without a resample */
} msseg_restore_desc;
int msseg_restore_native_u8(const void* src, int src_is_logits, int C, const void* desc, uint8_t* dst, msseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MSSEG_H_ */
