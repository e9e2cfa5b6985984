// igemm_fwd_kernel instantiations: conv k3 s1 p1 on 4x8x16 tiles (k3_plan cfg 0), cout blocks 16 and 32, bf16.  These are the
// slowest instantiations to compile, hence one file per dtype.
#include "igemm_fwd_kernel.h"

int msseg_igemm_k3_big_bf16(IgemmParams& p, hipStream_t stream) { return launch_k3_big<bf16_t>(p, stream); }
