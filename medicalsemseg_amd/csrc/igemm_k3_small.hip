// igemm_fwd_kernel instantiations: conv k3 s1 p1 on 2x4x8 tiles (k3_plan cfg 2); cout blocks 16 / 32 / 48, both dtypes.
#include "igemm_fwd_kernel.h"

int msseg_igemm_k3_small(IgemmParams& p, int dtype, hipStream_t stream) {
    return launch_dtype<27, SRC_DIRECT, EPI_STORE, 2, 4, 8, 4>(p, dtype, stream);
}
