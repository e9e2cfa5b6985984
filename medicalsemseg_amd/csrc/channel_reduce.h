// What the per-channel streaming passes share (channel_reduce.hip, instnorm.hip, layernorm.hip, head_conv.hip, maxpool.hip,
// pointwise.hip): the chunk object of their kernels, the thread -> (row lane, channel group) map, the two-stage block
// reduction and the second launch that adds the blocks' partial rows.  All tensors channels-last with an explicit voxel
// stride; 16-byte vector accesses when the channel count allows (C % (16/sizeof(T)) == 0), scalar fallback otherwise.
#pragma once
#include "common.h"

// A chunk's floats as one object, filled and written by Chunk<T> of common.h.  The kernels here keep this member form:
// on plain float arrays they compile to different code (the struct member carries its own alias information).
template <typename T> struct ChunkV {
    static constexpr int EPC = DT<T>::EPC;
    float v[EPC];
    MSSEG_DEVFN void load(const T* p) { Chunk<T>::load(p, v); }
    MSSEG_DEVFN void store(T* p) const { Chunk<T>::store(p, v); }
};

static inline bool vec_ok(const void* p, long long ld, int C, int esz) {
    const int epc = 16 / esz;
    return (C % epc) == 0 && (ld % epc) == 0 && (((uintptr_t)p) & 15) == 0;
}

// Work decomposition shared by the per-(n, voxel, channel-group) passes: a block owns `rows_per_block`
// consecutive voxels of sample blockIdx.y; thread -> (row lane, channel group); channel group fixed per thread.
struct RowMap {
    int groups;       // channel groups per voxel
    int rows_par;     // voxel rows processed in parallel by a block
};
static inline RowMap row_map(int C, int width, int nthr = 256) {
    RowMap m;
    m.groups = ceil_div(C, width);
    if (m.groups > nthr) m.groups = nthr;
    m.rows_par = nthr / m.groups;
    if (m.rows_par < 1) m.rows_par = 1;
    return m;
}

static inline long long reduce_blocks(long long S, int rows_par, int N, int C, int nper) {
    // one block per CU in total (each keeps ~32 KB of loads in flight) keeps the finalising block's job small
    long long blocks = ceil_div_ll(S, (long long)rows_par * 8);
    long long cap = (long long)msseg_num_cus() / (N > 0 ? N : 1);
    if (cap < 1) cap = 1;
    const long long fit = (long long)(((size_t)16 << 20) / ((size_t)N * C * nper * 4));
    if (cap > fit) cap = fit;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return blocks;
}

// Reduction kernels run 512-thread blocks (8 waves per CU, one block per CU, 12+ loads in flight per thread): enough loads in flight to stream HBM
// while the number of partial rows the finalising block has to add stays at one per CU.
constexpr int RED_THREADS = 512;
constexpr int RED_STAGE2 = 16;

// two-stage fixed-order sum over the rows_par row slots of red[(k * groups + g) * W + e][2]; result in slot k = 0
template <int W>
MSSEG_DEVFN void block_rows_reduce(float* red, int groups, int rows_par, int g, int rl, bool act) {
    if (act && rl < RED_STAGE2 && rl < rows_par) {
#pragma unroll
        for (int e = 0; e < W; ++e) {
            float a = 0.f, b = 0.f;
            for (int k = rl; k < rows_par; k += RED_STAGE2) {
                a += red[((k * groups + g) * W + e) * 2 + 0];
                b += red[((k * groups + g) * W + e) * 2 + 1];
            }
            red[((rl * groups + g) * W + e) * 2 + 0] = a;
            red[((rl * groups + g) * W + e) * 2 + 1] = b;
        }
    }
    __syncthreads();
}

// Second step of every channel reduction: 256-thread blocks (one per 256 columns, and per sample for statistics) add the
// per-block partial rows in a fixed order.  A
// separate launch -- the kernel boundary makes the rows visible, where an in-kernel "last block finalises" pays an
// agent-scope release (L2 write-back) per block plus an acquire: ~10-15 us per reduction on these sizes.
// Layout of ws and the three modes: finalize_channels (channel_reduce.hip).
struct FinalizeArgs {
    const float* ws; int N, nblk, C, nper, mode; float* out; float* dp0; float* dp1; int accumulate;
};
// launches channels_finalize_kernel (channel_reduce.hip) on `st`, behind the launch that wrote the rows
int msseg_channels_finalize_launch(const FinalizeArgs& a, hipStream_t st);
