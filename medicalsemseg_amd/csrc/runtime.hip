// What the whole library shares at run time: the per-thread error string, the ABI version, the device's CU count and
// the size of the reduce scratch.
#include "common.h"

#include <stdarg.h>

// ---------------------------------------------------------------------------------------------------------
// error plumbing / device info
// ---------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void msseg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" {
int msseg_abi_version(void) { return MSSEG_ABI_VERSION; }
const char* msseg_last_error(void) { return g_err; }
int msseg_num_cus(void) {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}

size_t msseg_reduce_scratch_bytes(void) { return ((size_t)16 << 20) + MSSEG_SCRATCH_HEADER_BYTES; }
}
