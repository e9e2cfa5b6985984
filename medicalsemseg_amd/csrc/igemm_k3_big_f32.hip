// igemm_fwd_kernel instantiations: conv k3 s1 p1 on 4x8x16 tiles (k3_plan cfg 0), cout blocks 16 and 32, fp32.  These are the
// slowest instantiations to compile, hence one file per dtype.
#include "igemm_fwd_kernel.h"

int msseg_igemm_k3_big_f32(IgemmParams& p, hipStream_t stream) { return launch_k3_big<float>(p, stream); }
