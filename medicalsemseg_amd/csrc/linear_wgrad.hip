// Weight and bias gradient of a Linear layer on many tokens (bf16) in one pass over the tokens, for gfx950.
//
//   dW[m][k] = sum_t dy[t][m] * x[t][k]        db[m] = sum_t dy[t][m]
//
// Replaces, for nn.Linear in the Swin stages (qkv / proj / fc1 / fc2 of /root/reference/models/backbones/swin_nnformer.py:
// 24-42,128-196; 221 k tokens x 48 ... 192 channels in the first stage), autograd's weight.grad = dy^T x and
// bias.grad = dy.sum(0).  The generic flat kernel (igemm_wgrad.hip) gives every (32 x 32) output block pair its own
// workgroup column, each of which walks ALL tokens reading its 64-byte slices of the rows -- ten columns for 48 -> 144,
// 87 us where the tensors are 85 MB (10.6 us at 8 TB/s) -- and the bias gradient was one more pass over dy
// (msseg_channel_sum, 28 us).  Here a workgroup reads WHOLE token rows (its slice of the output: NTP x NTQ 16-wide
// tiles, up to 192 x 48 / 48 x 192 / 96 x 96, usually the whole layer), keeps its partial dW in registers across all
// its token chunks, gets db from one more MFMA per row tile against a fragment of ones, and writes ONE partial block;
// a second small kernel adds the workgroups' blocks in a fixed order (deterministic) into the torch-layout gradients.
//
// The kernel itself (wgrad_onepass.h) takes the dy row of a token from a row source: plain rows for nn.Linear, the gathered child
// rows of a transposed convolution for msseg_lwg_deconv_wgrad below (k2 s2) and for deconv_k4s4.hip (k4 s4).
#include "wgrad_onepass.h"

namespace {

struct LwgRedParams {
    const float* part;
    float* dw; float* db;
    int M, K, ntp16, ntq16, mslices, kslices, nwg, acc_w, acc_b;
    int stride;     // floats between the partial blocks of two workgroups (lwg_part_floats)
    int dcv_cout;   // > 0: m = abc * cout + co of a transposed conv: dw in the torch layout [K = Cin][cout][8]
};

// 256 threads = 32 outputs x 8 groups: a thread adds every 8th workgroup's partial (8 loads in flight), the 8 group sums are
// added through LDS in a fixed order (deterministic)
__global__ __launch_bounds__(256) void lwg_reduce_kernel(const LwgRedParams p) {
    __shared__ float gs[8][33];
    const int total = p.M * p.K + (p.db ? p.M : 0);
    const int part = p.stride;
    const int ol = threadIdx.x & 31, sg = threadIdx.x >> 5;
    for (int base = blockIdx.x * 32; base < total; base += gridDim.x * 32) {
        const int i = base + ol;
        float s = 0.f;
        bool bias = false;
        int m = 0;
        if (i < total) {
            bias = i >= p.M * p.K;
            m = bias ? i - p.M * p.K : i / p.K;
            const int k = bias ? 0 : i - m * p.K;
            const int ms = m / p.ntp16, ml = m - ms * p.ntp16, ks = k / p.ntq16, kl = k - ks * p.ntq16;
            const float* src = p.part + (long long)(ms * p.kslices + ks) * p.nwg * part + (bias ? p.ntp16 * p.ntq16 + ml : kl * p.ntp16 + ml);
            int w = sg;
            for (; w + 56 < p.nwg; w += 64) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = src[(long long)(w + 8 * j) * part];
#pragma unroll
                for (int j = 0; j < 8; ++j) s += v[j];
            }
            for (; w < p.nwg; w += 8) s += src[(long long)w * part];
        }
        gs[sg][ol] = s;
        __syncthreads();
        if (sg == 0 && i < total) {
            float tot = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) tot += gs[j][ol];
            if (bias) {
                p.db[m] = p.acc_b ? p.db[m] + tot : tot;
            } else if (p.dcv_cout > 0) {
                const int k = i - m * p.K, abc = m / p.dcv_cout, co = m - abc * p.dcv_cout;
                float* o = p.dw + ((long long)k * p.dcv_cout + co) * 8 + abc;
                *o = p.acc_w ? *o + tot : tot;
            } else {
                p.dw[i] = p.acc_w ? p.dw[i] + tot : tot;
            }
        }
        __syncthreads();
    }
}

// slice shapes with an instantiation, in order of preference (most output tiles per workgroup first)
struct Shape { int ntp, ntq; };
constexpr Shape kShapes[] = {{12, 3}, {3, 12}, {6, 6}, {9, 3}, {3, 9}, {6, 3}, {3, 6}, {3, 3}};
// transposed convs: 8 * Cout / 16 is a multiple of 4, so a multiple of 3 is one of 12.  Measured (tools/bench_deconv.py, B = 2):
// 48 -> 48 on 221 k coarse voxels 96 -> 63 us against the generic flat kernel, but 64 -> 32 on 27 k voxels 18 -> 28 us and
// 128 -> 64 on 3.5 k 14 -> 21 us (power-of-two shapes {8, 4} / {8, 2}, since removed): with a few chunks per workgroup the
// partial blocks and their reduction cost more than the flat kernel's re-reads.  Only the 48-multiples on large grids come here.
constexpr Shape kShapesDcv[] = {{12, 3}};

bool pick_shape(const Shape* shapes, int n, int M, int K, Shape* out) {
    if (M % 16 || K % 16) return false;
    const int tm = M / 16, tk = K / 16;
    for (int i = 0; i < n; ++i)
        if (tm % shapes[i].ntp == 0 && tk % shapes[i].ntq == 0) { *out = shapes[i]; return true; }
    return false;
}
bool pick_shape_dcv(int M, int K, Shape* out) { return pick_shape(kShapesDcv, sizeof(kShapesDcv) / sizeof(Shape), M, K, out); }
bool pick_shape(int M, int K, Shape* out) { return pick_shape(kShapes, sizeof(kShapes) / sizeof(Shape), M, K, out); }

// the kernel (through `launch(gx, slices)`) on M x K outputs in slices of shape s, then the fixed-order sum of the partial blocks
// into dw (and db: the row source accumulates bias sums)
template <class Launch>
int run_lwg(LwgParams& p, Shape s, int M, int K, bool bias_sums, float* dw, float* db, int acc_w, int acc_b, int dcv_cout,
            void* workspace, size_t workspace_bytes, const char* who, hipStream_t stream, Launch launch) {
    const int mslices = M / (s.ntp * 16), slices = mslices * (K / (s.ntq * 16));
    const int part = s.ntp * 16 * s.ntq * 16 + (bias_sums ? s.ntp * 16 : 0);   // lwg_part_floats
    p.kslices = K / (s.ntq * 16);
    p.nchunks = (int)((p.NV + LWG_TT - 1) / LWG_TT);
    p.part = (float*)workspace;
    const size_t slice_bytes = (size_t)part * 4 * slices;
    if (workspace_bytes < slice_bytes) MSSEG_FAIL(MSSEG_EWORKSPACE, "%s: workspace %zu B too small (need >= %zu)", who, workspace_bytes, slice_bytes);
    const int gx = lwg_grid_x(slices, p.nchunks, workspace_bytes / slice_bytes);
    if (int rc = launch(gx, slices)) return rc;
    LwgRedParams r{};
    r.part = p.part; r.dw = dw; r.db = db; r.M = M; r.K = K; r.ntp16 = s.ntp * 16; r.ntq16 = s.ntq * 16;
    r.mslices = mslices; r.kslices = p.kslices; r.nwg = gx; r.acc_w = acc_w; r.acc_b = acc_b; r.stride = part; r.dcv_cout = dcv_cout;
    int rb = (M * K + (db ? M : 0) + 31) / 32;
    if (rb > 4096) rb = 4096;
    hipLaunchKernelGGL(lwg_reduce_kernel, dim3(rb), dim3(256), 0, stream, r);
    MSSEG_CHECK_LAUNCH(who);
    return MSSEG_OK;
}

}  // namespace

// ---- weight gradient of ConvTranspose3d k2 s2 on the one-pass kernel (called by msseg_deconv_k2s2_wgrad, igemm_wgrad.hip):
// dw[Cin][Cout][2][2][2] (+)= sum over coarse voxels of x[v][ci] * dy[child abc of v][co].  The generic flat kernel gave every
// (32 x 32) block pair of the [Cin][8 * Cout] matrix its own workgroup column, each walking all voxels (34 us per BasicUNet
// layer, 64 us per Swin-UNETR layer); here a workgroup reads whole rows -- the coarse row and the 8 child rows it gathers.
bool msseg_lwg_deconv_ok(int dtype, long long NV, int Cin, int Cout, const void* x, long long ldx, const void* dy, long long lddy) {
    Shape s;
    if (NV < 100000 || NV > 0x7fffffffLL / 8 || Cout % 8 || !msseg_aligned_bf16(dtype, x, ldx, Cin, dy, lddy, Cout)) return false;
    return pick_shape_dcv(8 * Cout, Cin, &s);
}

int msseg_lwg_deconv_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw, int N, int D, int H, int W,
                           int Cin, int Cout, int accumulate, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    Shape s;
    if (!pick_shape_dcv(8 * Cout, Cin, &s)) MSSEG_FAIL(MSSEG_EINVAL, "deconv wgrad: shape %d -> %d has no instantiation", Cin, Cout);
    if ((uintptr_t)workspace & 15) MSSEG_FAIL(MSSEG_EINVAL, "deconv wgrad: workspace alignment");
    LwgParams p{};
    p.x = x; p.ldx = ldx; p.dy = dy; p.lddy = lddy; p.NV = (long long)N * D * H * W;
    p.D = D; p.H = H; p.W = W; p.cout = Cout;
    const char* who = "deconv wgrad";
    return run_lwg(p, s, 8 * Cout, Cin, false, dw, nullptr, accumulate, 0, Cout, workspace, workspace_bytes, who, stream,
                   [&](int gx, int slices) {   // kShapesDcv
                       return lwg_launch<12, 3, RowsDeconvK2<12, 3>>(p, gx, slices, who, stream);
                   });
}

extern "C" {

int msseg_linear_wgrad_ok(long long NV, int Cin, int Cout, int dtype) {
    Shape s;
    if (dtype != MSSEG_BF16 || NV < 1 || NV > 0x7fffffffLL || Cin > 4096 || Cout > 4096) return 0;
    // a few hundred tokens against a large weight (last Swin stage): the partial blocks dominate, the generic kernel + channel
    // sum measured 3 us faster per layer (tools/bench_linear.py: 432 tokens, 384 -> 1152 / 1536, 1536 -> 384)
    if (NV < 1024 && (long long)Cin * Cout > 200000) return 0;
    return pick_shape(Cout, Cin, &s) ? 1 : 0;
}

int msseg_linear_wgrad(const void* x, long long ldx, const void* dy, long long lddy, float* dw, float* dbias, long long NV,
                       int Cin, int Cout, int accumulate_w, int accumulate_b, void* workspace, size_t workspace_bytes,
                       int dtype, msseg_stream_t stream) {
    if (!x || !dy || !dw || !workspace) MSSEG_FAIL(MSSEG_EINVAL, "linear_wgrad: null pointer");
    if (!msseg_linear_wgrad_ok(NV, Cin, Cout, dtype)) MSSEG_FAIL(MSSEG_EINVAL, "linear_wgrad: shape %d -> %d not supported (msseg_linear_wgrad_ok)", Cin, Cout);
    if (!msseg_aligned_bf16(dtype, x, ldx, Cin, dy, lddy, Cout) || ((uintptr_t)workspace & 15))
        MSSEG_FAIL(MSSEG_EINVAL, "linear_wgrad: operands must be 16-byte aligned with 16-byte row strides");
    Shape s;
    pick_shape(Cout, Cin, &s);
    LwgParams p{};
    p.x = x; p.ldx = ldx; p.dy = dy; p.lddy = lddy; p.NV = NV;
    const char* who = "linear_wgrad";
    hipStream_t st = (hipStream_t)stream;
    return run_lwg(p, s, Cout, Cin, true, dw, dbias, accumulate_w, accumulate_b, 0, workspace, workspace_bytes, who, st,
                   [&](int gx, int slices) {   // kShapes
                       switch (s.ntp * 100 + s.ntq) {
                           case 1203: return lwg_launch<12, 3, RowsPlain<12, 3>>(p, gx, slices, who, st);
                           case 312: return lwg_launch<3, 12, RowsPlain<3, 12>>(p, gx, slices, who, st);
                           case 606: return lwg_launch<6, 6, RowsPlain<6, 6>>(p, gx, slices, who, st);
                           case 903: return lwg_launch<9, 3, RowsPlain<9, 3>>(p, gx, slices, who, st);
                           case 309: return lwg_launch<3, 9, RowsPlain<3, 9>>(p, gx, slices, who, st);
                           case 603: return lwg_launch<6, 3, RowsPlain<6, 3>>(p, gx, slices, who, st);
                           case 306: return lwg_launch<3, 6, RowsPlain<3, 6>>(p, gx, slices, who, st);
                           case 303: return lwg_launch<3, 3, RowsPlain<3, 3>>(p, gx, slices, who, st);
                       }
                       return (int)MSSEG_EINVAL;
                   });
}

}  // extern "C"
