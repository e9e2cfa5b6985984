// igemm_fwd_kernel instantiations: the flat 1-tap GEMM families (one "tile" = 256 consecutive output voxels), both dtypes.
#include "igemm_fwd_kernel.h"

// direct source, plain store (conv k1 / Linear and its input gradient with fused sums); cout blocks 16 / 32 / 48
int msseg_igemm_flat(IgemmParams& p, int dtype, hipStream_t stream) {
    return launch_dtype<1, SRC_DIRECT, EPI_STORE, 1, 1, 256, 4>(p, dtype, stream);
}

// im2col gather source (few-channel convs); cout blocks 16 / 32 / 48
int msseg_igemm_gather(IgemmParams& p, int dtype, hipStream_t stream) {
    return launch_dtype<1, SRC_GATHER, EPI_STORE, 1, 1, 256, 4>(p, dtype, stream);
}

// the children of a ConvTranspose k2 s2 as source (its input gradient); cout blocks 16 / 32 / 48
int msseg_igemm_deconv_bwd(IgemmParams& p, int dtype, hipStream_t stream) {
    return launch_dtype<1, SRC_DECONV_BWD, EPI_STORE, 1, 1, 256, 4>(p, dtype, stream);
}

namespace {

// ConvTranspose k2 s2 pixel-shuffle epilogue: launch_nt with the 32-wide block only.  The one caller of msseg_igemm_deconv is
// msseg_deconv_k2s2_fwd (igemm_fwd.hip), the only user of EPI_DECONV: it rejects Cout % 4 != 0, leaves p.cout_block at 0 and
// sets p.M = 8 * Cout, a multiple of 32 that is at least 32, for which msseg_cout_block returns 32.  The 16- and 48-wide
// instantiations could never be launched.
template <typename T> int launch_deconv(IgemmParams& p, hipStream_t stream) {
    const int cb = p.cout_block ? p.cout_block : msseg_cout_block(p.M);
    if (cb == 32) return launch_cfg<T, 1, SRC_DIRECT, EPI_DECONV, 1, 1, 256, 4, 2>(p, stream);
    MSSEG_FAIL(MSSEG_EINVAL, "igemm: bad cout block %d", cb);
}

}  // namespace

int msseg_igemm_deconv(IgemmParams& p, int dtype, hipStream_t stream) {
    int rc = MSSEG_OK;
    if (!for_dtype(dtype, [&](auto t) { rc = launch_deconv<typename decltype(t)::type>(p, stream); }))
        MSSEG_FAIL(MSSEG_EINVAL, "igemm: bad dtype %d", dtype);
    return rc;
}
