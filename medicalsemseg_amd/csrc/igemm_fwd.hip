// Host side of the implicit-GEMM forward-shaped convolutions: the conv k3 tile / cout-block plan, the second step of the
// fused epilogue reductions, argument validation and the C entry points.  The kernel and its launch templates are in
// igemm_fwd_kernel.h, its instantiations in the igemm_*.hip files behind the msseg_igemm_* launchers (k3pp.h).
#include "igemm_fwd_kernel.h"

namespace {

// second step of the fused epilogue reductions: see msseg_k3_fused_finalize (k3pp.h); R = partial rows per cout block
__global__ __launch_bounds__(256) void k3_stats_finalize_kernel(const K3Fused f, int R, int N, int coutb, int M, bool inbwd) {
    __shared__ __attribute__((aligned(16))) float fin[256 * 4 + 8 * 48 * 2];
    const int tid = threadIdx.x;
    const int L = N * coutb * 2;
    const int cbase = blockIdx.x * coutb;
    if (!inbwd) {
        // forward statistics: one block per (cout block, sample) sums that sample's column slice of the partial rows
        // (with one block per cout block a thread walked 64 ... 128 rows: 5 us at N = 2, 8 us at N = 8)
        const int n = blockIdx.y, Ls = coutb * 2;
        block_rows_sum<256>(f.stats_ws + (long long)blockIdx.x * R * L + n * Ls, R, Ls, fin, L);
        const float* tot = fin + 256 * 4;   // [cl][2]
        for (int i = tid; i < Ls; i += 256) {
            const int cl = i >> 1, k = i & 1;
            if (cbase + cl < M) f.stats[((long long)n * M + cbase + cl) * 2 + k] = tot[i];
        }
        return;
    }
    block_rows_sum<256>(f.stats_ws + (long long)blockIdx.x * R * L, R, L, fin);
    const float* tot = fin + 256 * 4;   // [n][cl][2]
    if (tid < coutb && cbase + tid < M) {
        // sum dz*xhat = rstd * (sum dz*yraw - mean * sum dz); dbeta / dgamma = sums over the samples
        const int cg = cbase + tid;
        float g0 = 0.f, g1 = 0.f;
        const float inv = 1.0f / (float)f.nb_S;
        for (int nn = 0; nn < N; ++nn) {
            const float a = tot[(nn * coutb + tid) * 2], b0 = tot[(nn * coutb + tid) * 2 + 1];
            const float fs = f.nb_stats[((long long)nn * M + cg) * 2], fs2 = f.nb_stats[((long long)nn * M + cg) * 2 + 1];
            const float mean = fs * inv;
            float var = fs2 * inv - mean * mean;
            var = var > 0.f ? var : 0.f;
            const float b2 = rsqrtf(var + f.nb_eps) * (b0 - mean * a);
            g0 += a;
            g1 += b2;
            f.stats[((long long)nn * M + cg) * 2 + 0] = a;
            f.stats[((long long)nn * M + cg) * 2 + 1] = b2;
        }
        if (f.nb_dgamma != nullptr) {
            f.nb_dbeta[cg] = f.nb_acc ? f.nb_dbeta[cg] + g0 : g0;
            f.nb_dgamma[cg] = f.nb_acc ? f.nb_dgamma[cg] + g1 : g1;
        }
    }
}

// Tile / cout-block choice for a conv k3 problem: the largest tile that still yields >= ~3/4 of a chip of
// workgroups; tiny grids (6^3 .. 12^3 with many channels) drop to 16-wide cout blocks to expose more parallelism
// (those layers are latency-bound chains of weight-block loads, not MFMA-bound).  cfg: 0 big, 1 mid, 2 small.
static void k3_plan(int N, int D, int H, int W, int M, int* cfg, int* cb) {
    const int mn = D < H ? (D < W ? D : W) : (H < W ? H : W);
    const int std_cb = msseg_cout_block(M);
    const long long want = (long long)msseg_num_cus() * 3 / 4;
    auto wgs = [&](int td, int th, int tw, int c) {
        return (long long)N * ceil_div(D, td) * ceil_div(H, th) * ceil_div(W, tw) * ceil_div(M, c);
    };
    if (mn >= 32 && wgs(4, 8, 16, std_cb) >= want) {
        *cfg = 0;
        // the 48-wide (NT = 3) instantiation of the big tile spills (142 VGPRs): two 32-wide blocks, the second half
        // empty, measured faster at 96^3 (48->48: 488 vs 633 us, 96->48: 731 vs 948 us; 16-wide blocks: 491 / 778 us)
        *cb = (std_cb == 48) ? 32 : std_cb;
        return;
    }
    if (mn >= 12 && wgs(4, 4, 8, std_cb) >= want) { *cfg = 1; *cb = std_cb; return; }
    *cfg = 2;
    *cb = (wgs(2, 4, 8, std_cb) >= want || std_cb == 16) ? std_cb : 16;
}

// dtype: MSSEG_F32 or MSSEG_BF16 (check_common has run)
int launch_k3(IgemmParams& p, int dtype, hipStream_t stream) {
    int cfg, cb;
    k3_plan(p.N, p.D, p.H, p.W, p.M, &cfg, &cb);
    p.cout_block = cb;
    // a tap-sliced variant of the big tile with two workgroups per CU measured 144 vs 110 us (32->32 at 96^3) and was removed
    if (cfg == 0) return dtype == MSSEG_F32 ? msseg_igemm_k3_big_f32(p, stream) : msseg_igemm_k3_big_bf16(p, stream);
    if (cfg == 1) return msseg_igemm_k3_mid(p, dtype, stream);
    return msseg_igemm_k3_small(p, dtype, stream);
}

// the operands every entry point passes on; the caller adds the grid and what its source mode / epilogue needs
IgemmParams igemm_params(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy, int K, int M) {
    IgemmParams p{};
    p.x = x; p.ldx = ldx; p.wp = wp; p.bias = bias; p.y = y; p.ldy = ldy;
    p.K = K; p.M = M;
    return p;
}

int check_common(const void* x, long long ldx, const void* wp, const void* y, long long ldy, int dtype, int esz) {
    if (!x || !wp || !y) MSSEG_FAIL(MSSEG_EINVAL, "igemm: null pointer");
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "igemm: bad dtype %d", dtype);
    if (((uintptr_t)x | (uintptr_t)wp) & 15) MSSEG_FAIL(MSSEG_EINVAL, "igemm: x/wp must be 16-byte aligned");
    if ((ldx * esz) % 16) MSSEG_FAIL(MSSEG_EINVAL, "igemm: ldx*elem must be a multiple of 16 bytes");
    (void)ldy;
    return MSSEG_OK;
}

}  // namespace

int msseg_k3_fused_finalize(const K3Fused& f, int gx, int N, int coutb, int M, bool inbwd, int ncb, hipStream_t stream) {
    hipLaunchKernelGGL(k3_stats_finalize_kernel, dim3(ncb, inbwd ? 1 : N), dim3(256), 0, stream, f, gx, N, coutb, M, inbwd);
    MSSEG_CHECK_LAUNCH("k3_stats_finalize");
    return MSSEG_OK;
}

extern "C" {

int msseg_cout_block(int M) {
    if (M <= 16) return 16;
    if (M % 32 == 0) return 32;
    if (M % 48 == 0) return 48;
    return 32;
}

int msseg_conv3d_k3_cout_block(int N, int D, int H, int W, int Cout) {
    int cfg, cb;
    k3_plan(N, D, H, W, Cout, &cfg, &cb);
    return cb;
}

int msseg_conv3d_k3_variant(int N, int D, int H, int W, int Cout) {
    int cfg, cb;
    k3_plan(N, D, H, W, Cout, &cfg, &cb);
    return cfg;
}

int msseg_conv3d_k3_kernel(int N, int D, int H, int W, int Cin, int Cout, int dtype) {
    int cfg, cb;
    if (dtype == MSSEG_BF16 && Cin == 48 && msseg_k3c48_shape_ok(N, D, H, W, Cout)) return 4;
    k3_plan(N, D, H, W, Cout, &cfg, &cb);
    if (dtype == MSSEG_BF16 && cb == 32) {
        K3ppParams pp{};
        pp.x = (const void*)256; pp.y = (void*)256; pp.ldx = Cin; pp.ldy = Cout;
        pp.N = N; pp.D = D; pp.H = H; pp.W = W; pp.K = Cin; pp.M = Cout;
        if ((Cin % 8) == 0 && (Cout % 4) == 0 && msseg_k3pp_eligible(pp)) return 3;
    }
    return cfg;
}

int msseg_conv3d_k3_resident_per_cu(int N, int D, int H, int W, int Cin, int Cout, int dtype) {
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_resident_per_cu: bad dtype %d", dtype);
    if (N < 1 || D < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_resident_per_cu: bad shape");
    if (msseg_conv3d_k3_kernel(N, D, H, W, Cin, Cout, dtype) > 2)
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_resident_per_cu: the problem runs on a ping-pong kernel, not on the generic one");
    // the launch path itself up to the launch: same plan, same instantiation, same LDS size
    int resident = 0;
    IgemmParams p = igemm_params(nullptr, Cin, nullptr, nullptr, nullptr, Cout, Cin, Cout);
    p.N = N; p.D = D; p.H = H; p.W = W;
    p.resident_out = &resident;
    const int rc = launch_k3(p, dtype, nullptr);
    return rc ? rc : resident;
}

// conv k3 p1 with the optional fused reductions f (f.stats == nullptr: none); stats_ws and nb_S are filled in here
static int k3_fwd_impl(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy, int N,
                       int D, int H, int W, int Cin, int Cout, K3Fused f, void* scratch, size_t scratch_bytes, int dtype,
                       msseg_stream_t stream) {
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    int rc = check_common(x, ldx, wp, y, ldy, dtype, esz);
    if (rc) return rc;
    if (N < 1 || D < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3: bad shape");
    if (Cin % (16 / esz)) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3: Cin=%d must be a multiple of %d (use conv3d_gather)", Cin, 16 / esz);
    if (ldx < Cin || ldy < Cout) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3: ld smaller than channels");
    if (f.stats) {
        if (N > MSSEG_STATS_NMAX) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3: fused statistics need N <= %d", MSSEG_STATS_NMAX);
        if (Cout > 64 * 16) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3: fused statistics need Cout <= 1024");
        if ((rc = scratch_ok(scratch, scratch_bytes, "conv3d_k3 (fused statistics)"))) return rc;
        f.stats_ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
        f.nb_S = (long long)D * H * W;
    }
    if (dtype == MSSEG_BF16) {
        // the 32-input-channel layers (the 96^3 / 48^3 levels) run on the ping-pong kernel when the grid is large enough
        K3ppParams pp{};
        pp.x = x; pp.ldx = ldx; pp.wp = wp; pp.bias = bias; pp.y = y; pp.ldy = ldy;
        pp.N = N; pp.D = D; pp.H = H; pp.W = W; pp.K = Cin; pp.M = Cout;
        pp.fused = f;
        if (Cin == 48 && msseg_k3c48_shape_ok(N, D, H, W, Cout)) {
            // the packed image is the four-part one of the 48-channel kernel (msseg_conv3d_k3_kernel() == 4): no fallback
            if (!msseg_k3c48_eligible(pp))
                MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3: 48-input-channel layer on a large grid needs 16-byte aligned x, 8-byte "
                                         "aligned y and ldx <= 256");
            return msseg_k3c48_launch(pp, (hipStream_t)stream);
        }
        int cfg, cb;
        k3_plan(N, D, H, W, Cout, &cfg, &cb);   // the packed weight image must be the 32-wide one
        if (cb == 32 && msseg_k3pp_eligible(pp)) return msseg_k3pp_launch(pp, (hipStream_t)stream);
    }
    IgemmParams p = igemm_params(x, ldx, wp, bias, y, ldy, Cin, Cout);
    p.N = N; p.D = D; p.H = H; p.W = W;
    p.fused = f;
    return launch_k3(p, dtype, (hipStream_t)stream);
}

int msseg_conv3d_k3_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                        int N, int D, int H, int W, int Cin, int Cout, float* stats, void* scratch,
                        size_t scratch_bytes, int dtype, msseg_stream_t stream) {
    K3Fused f{};
    f.stats = stats;
    return k3_fwd_impl(x, ldx, wp, bias, y, ldy, N, D, H, W, Cin, Cout, f, scratch, scratch_bytes, dtype, stream);
}

int msseg_conv3d_k3_fwd_accumulate(const void* x, long long ldx, const void* wp, void* y, long long ldy, int N, int D, int H,
                                   int W, int Cin, int Cout, float* stats, void* scratch, size_t scratch_bytes, int dtype,
                                   msseg_stream_t stream) {
    if (!x || !wp || !y || !stats) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_accumulate: null pointer");
    if (dtype != MSSEG_BF16 || N < 1 || N > MSSEG_STATS_NMAX) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_accumulate: bf16, N <= %d", MSSEG_STATS_NMAX);
    if (int rc = scratch_ok(scratch, scratch_bytes, "conv3d_k3_fwd_accumulate")) return rc;
    K3ppParams pp{};
    pp.x = x; pp.ldx = ldx; pp.wp = wp; pp.y = y; pp.ldy = ldy;
    pp.N = N; pp.D = D; pp.H = H; pp.W = W; pp.K = Cin; pp.M = Cout;
    pp.fused.stats = stats;
    pp.fused.stats_ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    pp.accumulate = 1;
    if (Cin == 48) {
        if (!msseg_k3c48_eligible(pp))
            MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_accumulate: 48 input channels need a shape and operands the 48-channel "
                                     "kernel takes (msseg_conv3d_k3_kernel() == 4, 16-byte aligned x, N <= 4)");
        return msseg_k3c48_launch(pp, (hipStream_t)stream);
    }
    if (!msseg_k3pp_eligible(pp))
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_accumulate: only shapes of the ping-pong kernel (32 input channels, Cout %% 32 == 0, "
                                 "large grids; msseg_conv3d_k3_kernel() == 3)");
    return msseg_k3pp_launch(pp, (hipStream_t)stream);
}

int msseg_conv3d_k3_split_ok(int N, int D, int H, int W, int Cin, int Cout, int split, int dtype) {
    if (N < 1 || D < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return 0;
    if (Cout % 32 || split <= 0 || split >= Cout || split % 32) return 0;
    return msseg_conv3d_k3_kernel(N, D, H, W, Cin, Cout, dtype) == 3;
}

int msseg_conv3d_k3_fwd_split(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                              void* y2, long long ldy2, int split, int N, int D, int H, int W, int Cin, int Cout,
                              float* stats, int accumulate, int dtype, msseg_stream_t stream) {
    if (int rc = check_common(x, ldx, wp, y, ldy, dtype, dtype == MSSEG_F32 ? 4 : 2)) return rc;
    if (!y2) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_split: null pointer");
    if (stats || accumulate)
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_split: two destinations come with the plain epilogue only (no fused statistics, no accumulate)");
    if (!msseg_conv3d_k3_split_ok(N, D, H, W, Cin, Cout, split, dtype))
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_split: only problems of the ping-pong kernel (msseg_conv3d_k3_kernel() == 3) with "
                                 "0 < split < Cout on a 32-channel boundary (split=%d, Cout=%d)", split, Cout);
    if (ldx < Cin || ldy < split || ldy2 < Cout - split) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_split: ld smaller than channels");
    K3ppParams pp{};
    pp.x = x; pp.ldx = ldx; pp.wp = wp; pp.bias = bias; pp.y = y; pp.ldy = ldy;
    pp.y2 = y2; pp.ldy2 = ldy2; pp.split_cb = split / 32;
    pp.N = N; pp.D = D; pp.H = H; pp.W = W; pp.K = Cin; pp.M = Cout;
    if (!msseg_k3pp_eligible(pp))
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_fwd_split: the ping-pong kernel needs 16-byte aligned x and bias, 8-byte aligned y / y2 "
                                 "and row lengths that are multiples of 4 elements");
    return msseg_k3pp_launch(pp, (hipStream_t)stream);
}

int msseg_conv3d_k3_dgrad_inbwd(const void* dy, long long lddy, const void* wp, void* da, long long ldda, int N, int D,
                                int H, int W, int Cin, int Cout, const void* yraw, long long ldyraw, const void* act,
                                long long ldact, const float* fwd_stats, float slope, float eps, float* red,
                                float* dgamma, float* dbeta, int accumulate, void* scratch, size_t scratch_bytes,
                                int dtype, msseg_stream_t stream) {
    if (!yraw || !act || !fwd_stats || !red) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_dgrad_inbwd: null pointer");
    if ((dgamma == nullptr) != (dbeta == nullptr)) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_dgrad_inbwd: dgamma/dbeta go together");
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    if (Cout % 4 || (ldyraw % 4) || (ldact % 4) || ((uintptr_t)yraw % (4 * esz)) || ((uintptr_t)act % (4 * esz)))
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3_dgrad_inbwd: channel count / strides must be multiples of 4");
    K3Fused f{};
    f.stats = red;
    f.nb_y = yraw; f.nb_ldy = ldyraw; f.nb_a = act; f.nb_lda = ldact; f.nb_stats = fwd_stats;
    f.nb_slope = slope; f.nb_eps = eps;
    f.nb_dgamma = dgamma; f.nb_dbeta = dbeta; f.nb_acc = accumulate;
    return k3_fwd_impl(dy, lddy, wp, nullptr, da, ldda, N, D, H, W, Cin, Cout, f, scratch, scratch_bytes, dtype, stream);
}

int msseg_conv3d_k3s2_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                          int N, int ID, int IH, int IW, int Cin, int Cout, int dtype, msseg_stream_t stream) {
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    int rc = check_common(x, ldx, wp, y, ldy, dtype, esz);
    if (rc) return rc;
    if (N < 1 || ID < 1 || IH < 1 || IW < 1 || Cin < 1 || Cout < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3s2: bad shape");
    if (Cin % (16 / esz)) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k3s2: Cin=%d must be a multiple of %d", Cin, 16 / esz);
    IgemmParams p = igemm_params(x, ldx, wp, bias, y, ldy, Cin, Cout);
    p.N = N; p.ID = ID; p.IH = IH; p.IW = IW;
    p.D = (ID - 1) / 2 + 1; p.H = (IH - 1) / 2 + 1; p.W = (IW - 1) / 2 + 1;
    return msseg_igemm_k3s2(p, dtype, (hipStream_t)stream);
}

int msseg_conv3d_stem_norm_fwd(const void* x, long long ldx, const void* wp, const float* bias, const float* stats,
                               const float* gamma, const float* beta, float eps, float slope, void* y, long long ldy, int N,
                               int D, int H, int W, int Cout, int dtype, msseg_stream_t stream) {
    if (!x || !wp || !y || !stats || N < 1 || D < 1 || H < 1 || W < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_stem_norm: bad args");
    if (!msseg_stem_eligible(dtype, 1, Cout, 3, 1, 1, ldx, ldy, y))
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_stem_norm: bf16, Cout a multiple of 32 or 48 (<= 256), 8-byte aligned output rows only");
    StemParams sp{};
    sp.x = x; sp.ldx = ldx; sp.wp = wp; sp.bias = bias; sp.y = y; sp.ldy = ldy;
    sp.N = N; sp.D = D; sp.H = H; sp.W = W; sp.M = Cout;
    sp.nstats = stats; sp.gamma = gamma; sp.beta = beta; sp.eps = eps; sp.slope = slope;
    return msseg_stem_fwd_launch(sp, (hipStream_t)stream);
}

int msseg_conv3d_k1_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                        long long NV, int Cin, int Cout, int dtype, msseg_stream_t stream) {
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    int rc = check_common(x, ldx, wp, y, ldy, dtype, esz);
    if (rc) return rc;
    if (NV < 1 || NV > 0x7fffffffLL || Cin < 1 || Cout < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1: bad shape");
    if (Cin % (16 / esz)) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1: Cin=%d must be a multiple of %d", Cin, 16 / esz);
    // many tokens, few channels (the first Swin stage's Linear layers): register-resident-weight streaming kernel
    if (msseg_linear_regw_eligible(dtype, NV, Cin, Cout, x, ldx, y, ldy, bias))
        return msseg_linear_regw_launch(x, ldx, wp, bias, y, ldy, NV, Cin, Cout, (hipStream_t)stream);
    IgemmParams p = igemm_params(x, ldx, wp, bias, y, ldy, Cin, Cout);
    p.N = 1; p.D = 1; p.H = 1; p.W = (int)NV;
    return msseg_igemm_flat(p, dtype, (hipStream_t)stream);
}

int msseg_conv3d_gather_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                            int N, int ID, int IH, int IW, int Cin, int Cout, int k, int s, int pd, int dtype,
                            msseg_stream_t stream) {
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    if (!x || !wp || !y) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_gather: null pointer");
    if (dtype != MSSEG_F32 && dtype != MSSEG_BF16) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_gather: bad dtype");
    if (k < 1 || s < 1 || pd < 0 || Cin < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_gather: bad kernel geometry");
    const int OD = (ID + 2 * pd - k) / s + 1, OH = (IH + 2 * pd - k) / s + 1, OW = (IW + 2 * pd - k) / s + 1;
    if (OD < 1 || OH < 1 || OW < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_gather: empty output");
    const long long NV = (long long)N * OD * OH * OW;
    if (NV > 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_gather: too many voxels");
    if (msseg_stem_eligible(dtype, Cin, Cout, k, s, pd, ldx, ldy, y)) {
        StemParams sp{};
        sp.x = x; sp.ldx = ldx; sp.wp = wp; sp.bias = bias; sp.y = y; sp.ldy = ldy;
        sp.N = N; sp.D = ID; sp.H = IH; sp.W = IW; sp.M = Cout; sp.taps = k == 1 ? 1 : 27;
        return msseg_stem_fwd_launch(sp, (hipStream_t)stream);
    }
    IgemmParams p = igemm_params(x, ldx, wp, bias, y, ldy, Cin * k * k * k, Cout);
    p.N = 1; p.D = 1; p.H = 1; p.W = (int)NV;
    p.ID = ID; p.IH = IH; p.IW = IW; p.OD = OD; p.OH = OH; p.OW = OW;
    p.cin = Cin; p.k = k; p.s = s; p.p = pd;
    return msseg_igemm_gather(p, dtype, (hipStream_t)stream);
}

int msseg_conv3d_stem_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                          int N, int D, int H, int W, int Cout, int k, float* stats, void* scratch, size_t scratch_bytes,
                          int dtype, msseg_stream_t stream) {
    if (!x || !wp || (!y && !stats) || N < 1 || D < 1 || H < 1 || W < 1) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_stem: bad args");
    if (k != 1 && k != 3) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_stem: k = 1 (centre tap only) or 3, got %d", k);
    if (!msseg_stem_eligible(dtype, 1, Cout, 3, 1, 1, ldx, y ? ldy : 4, y))   // y == NULL: statistics only
        MSSEG_FAIL(MSSEG_EINVAL, "conv3d_stem: bf16, Cout a multiple of 32 or 48 (<= 256), 8-byte aligned output rows only");
    StemParams sp{};
    sp.x = x; sp.ldx = ldx; sp.wp = wp; sp.bias = bias; sp.y = y; sp.ldy = ldy;
    sp.N = N; sp.D = D; sp.H = H; sp.W = W; sp.M = Cout; sp.taps = k == 1 ? 1 : 27;
    if (stats) {
        if (N > MSSEG_STATS_NMAX) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_stem: fused statistics need N <= %d", MSSEG_STATS_NMAX);
        if (int rc = scratch_ok(scratch, scratch_bytes, "conv3d_stem (fused statistics)")) return rc;
        sp.stats = stats;
        sp.stats_ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    }
    return msseg_stem_fwd_launch(sp, (hipStream_t)stream);
}

int msseg_deconv_k2s2_fwd(const void* x, long long ldx, const void* wp, const float* bias, void* y, long long ldy,
                          int N, int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream) {
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    int rc = check_common(x, ldx, wp, y, ldy, dtype, esz);
    if (rc) return rc;
    if (Cin % (16 / esz) || Cout % 4) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2: Cin %% %d and Cout %% 4 must be 0", 16 / esz);
    const long long NV = (long long)N * D * H * W;
    if (NV < 1 || NV > 0x7fffffffLL / 8) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2: bad voxel count");
    if (msseg_deconv2_fast_eligible(dtype, Cin, Cout, x, ldx, y, ldy, bias))
        return msseg_deconv2_fwd_launch(x, ldx, wp, bias, y, ldy, N, D, H, W, Cin, Cout, (hipStream_t)stream);
    if (msseg_deconv2g_fwd_eligible(dtype, Cin, Cout, x, ldx, y, ldy, bias))
        return msseg_deconv2g_fwd_launch(x, ldx, wp, bias, y, ldy, N, D, H, W, Cin, Cout, (hipStream_t)stream);
    IgemmParams p = igemm_params(x, ldx, wp, bias, y, ldy, Cin, 8 * Cout);
    p.N = 1; p.D = 1; p.H = 1; p.W = (int)NV;
    p.OD = D; p.OH = H; p.OW = W; p.creal = Cout;
    return msseg_igemm_deconv(p, dtype, (hipStream_t)stream);
}

int msseg_deconv_k2s2_bwd_data(const void* dy, long long lddy, const void* wp, void* dx, long long lddx,
                               int N, int D, int H, int W, int Cin, int Cout, int dtype, msseg_stream_t stream) {
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    int rc = check_common(dy, lddy, wp, dx, lddx, dtype, esz);
    if (rc) return rc;
    if (Cout % (16 / esz)) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_data: Cout %% %d must be 0", 16 / esz);
    const long long NV = (long long)N * D * H * W;
    if (NV < 1 || NV > 0x7fffffffLL / 8) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_data: bad voxel count");
    if (msseg_deconv2_fast_eligible(dtype, Cin, Cout, dx, lddx, dy, lddy, nullptr))
        return msseg_deconv2_bwd_launch(dy, lddy, wp, dx, lddx, N, D, H, W, Cin, Cout, nullptr, 0, nullptr, 0, nullptr, 0.f, 0.f,
                                        nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, (hipStream_t)stream);
    if (msseg_deconv2g_bwd_eligible(dtype, Cin, Cout, dx, lddx, dy, lddy))
        return msseg_deconv2g_bwd_launch(dy, lddy, wp, dx, lddx, nullptr, N, D, H, W, Cin, Cout, (hipStream_t)stream);
    IgemmParams p = igemm_params(dy, lddy, wp, nullptr, dx, lddx, 8 * Cout, Cin);
    p.N = 1; p.D = 1; p.H = 1; p.W = (int)NV;
    p.OD = D; p.OH = H; p.OW = W; p.creal = Cout;
    return msseg_igemm_deconv_bwd(p, dtype, (hipStream_t)stream);
}

// ---- flat (1x1x1-tap) input-gradient kernels with the InstanceNorm-backward sums of the receiving layer fused into the
// epilogue, as msseg_conv3d_k3_dgrad_inbwd: the grid is tiled per sample (N samples of S voxels) so that a tile never
// straddles two samples.
static int flat_inbwd_common(IgemmParams& p, int N, long long S, int Cout, const void* yraw, long long ldyraw,
                             const void* act, long long ldact, const float* fwd_stats, float slope, float eps, float* red,
                             float* dgamma, float* dbeta, int accumulate, void* scratch, size_t scratch_bytes, int esz,
                             const char* who) {
    if (!yraw || !act || !fwd_stats || !red) MSSEG_FAIL(MSSEG_EINVAL, "%s: null pointer", who);
    if ((dgamma == nullptr) != (dbeta == nullptr)) MSSEG_FAIL(MSSEG_EINVAL, "%s: dgamma/dbeta go together", who);
    if (N < 1 || N > MSSEG_STATS_NMAX || S < 1 || S > 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "%s: 1 <= N <= %d samples", who, MSSEG_STATS_NMAX);
    if (Cout % 4 || (ldyraw % 4) || (ldact % 4) || ((uintptr_t)yraw % (4 * esz)) || ((uintptr_t)act % (4 * esz)))
        MSSEG_FAIL(MSSEG_EINVAL, "%s: channel count / strides must be multiples of 4", who);
    if (Cout > 64 * 16) MSSEG_FAIL(MSSEG_EINVAL, "%s: at most 1024 output channels", who);
    if (int rc = scratch_ok(scratch, scratch_bytes, who)) return rc;
    p.N = N; p.D = 1; p.H = 1; p.W = (int)S;
    p.fused.stats = red;
    p.fused.stats_ws = (float*)((unsigned char*)scratch + MSSEG_SCRATCH_HEADER_BYTES);
    p.fused.nb_y = yraw; p.fused.nb_ldy = ldyraw; p.fused.nb_a = act; p.fused.nb_lda = ldact; p.fused.nb_stats = fwd_stats;
    p.fused.nb_slope = slope; p.fused.nb_eps = eps; p.fused.nb_S = S;
    p.fused.nb_dgamma = dgamma; p.fused.nb_dbeta = dbeta; p.fused.nb_acc = accumulate;
    return MSSEG_OK;
}

int msseg_conv3d_k1_dgrad_inbwd(const void* dy, long long lddy, const void* wp, void* da, long long ldda, int N,
                                long long S, int Cin, int Cout, const void* yraw, long long ldyraw, const void* act,
                                long long ldact, const float* fwd_stats, float slope, float eps, float* red,
                                float* dgamma, float* dbeta, int accumulate, void* scratch, size_t scratch_bytes,
                                int dtype, msseg_stream_t stream) {
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    int rc = check_common(dy, lddy, wp, da, ldda, dtype, esz);
    if (rc) return rc;
    if (Cin < 1 || Cout < 1 || Cin % (16 / esz)) MSSEG_FAIL(MSSEG_EINVAL, "conv3d_k1_dgrad_inbwd: bad channel counts");
    IgemmParams p = igemm_params(dy, lddy, wp, nullptr, da, ldda, Cin, Cout);
    rc = flat_inbwd_common(p, N, S, Cout, yraw, ldyraw, act, ldact, fwd_stats, slope, eps, red, dgamma, dbeta, accumulate,
                           scratch, scratch_bytes, esz, "conv3d_k1_dgrad_inbwd");
    if (rc) return rc;
    return msseg_igemm_flat(p, dtype, (hipStream_t)stream);
}

int msseg_deconv_k2s2_bwd_fused(const void* dy, long long lddy, const void* wp, void* dx, long long lddx, int N,
                                int D, int H, int W, int Cin, int Cout, const void* yraw, long long ldyraw,
                                const void* act, long long ldact, const float* fwd_stats, float slope, float eps,
                                float* red, float* dgamma, float* dbeta, int accumulate, float* dbias, int dbias_accumulate,
                                void* scratch, size_t scratch_bytes, int dtype, msseg_stream_t stream) {
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    int rc = check_common(dy, lddy, wp, dx, lddx, dtype, esz);
    if (rc) return rc;
    if (Cout % (16 / esz)) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_fused: Cout %% %d must be 0", 16 / esz);
    const long long S = (long long)D * H * W;
    if ((long long)N * S > 0x7fffffffLL / 8) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_fused: bad voxel count");
    if (yraw) {
        if (!act || !fwd_stats || !red) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_fused: yraw needs act, fwd_stats and red");
        if (N > MSSEG_STATS_NMAX) MSSEG_FAIL(MSSEG_EINVAL, "deconv_k2s2_bwd_fused: fused sums need N <= %d", MSSEG_STATS_NMAX);
    }
    if (msseg_deconv2_fast_eligible(dtype, Cin, Cout, dx, lddx, dy, lddy, nullptr) &&
        (!yraw || ((ldyraw % 4) == 0 && (ldact % 4) == 0 && ((uintptr_t)yraw & 7) == 0 && ((uintptr_t)act & 7) == 0)))
        return msseg_deconv2_bwd_launch(dy, lddy, wp, dx, lddx, N, D, H, W, Cin, Cout, yraw, ldyraw, act, ldact, fwd_stats,
                                        slope, eps, red, dgamma, dbeta, accumulate, dbias, dbias_accumulate, scratch,
                                        scratch_bytes, (hipStream_t)stream);
    // generic path: the implicit-GEMM input gradient (with or without the fused sums) + a channel-sum pass for the bias
    if (yraw) {
        IgemmParams p = igemm_params(dy, lddy, wp, nullptr, dx, lddx, 8 * Cout, Cin);
        p.OD = D; p.OH = H; p.OW = W; p.creal = Cout;
        rc = flat_inbwd_common(p, N, S, Cin, yraw, ldyraw, act, ldact, fwd_stats, slope, eps, red, dgamma, dbeta, accumulate,
                               scratch, scratch_bytes, esz, "deconv_k2s2_bwd_fused");
        if (rc) return rc;
        rc = msseg_igemm_deconv_bwd(p, dtype, (hipStream_t)stream);
    } else {
        rc = msseg_deconv_k2s2_bwd_data(dy, lddy, wp, dx, lddx, N, D, H, W, Cin, Cout, dtype, stream);
    }
    if (rc) return rc;
    if (dbias)
        return msseg_channel_sum(dy, lddy, dbias, 8 * (long long)N * S, Cout, dbias_accumulate, scratch, scratch_bytes, dtype,
                                 stream);
    return MSSEG_OK;
}

}  // extern "C"
