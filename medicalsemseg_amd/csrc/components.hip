// Keep the largest connected component of every foreground class of a uint8 label map [D][H][W] on the device: MONAI's
// KeepLargestConnectedComponent(applied_labels=1..C-1, is_onehot=False, independent=True), also nnU-Net's post-processing.
// All classes are labelled at once (voxels of different classes are never united).  Integer work, lock-free, exact and
// bit-identical from run to run.
//
// Union-find on int32 labels L[v] that start as the voxel's own flat index; a union always hangs the larger root under the
// smaller one (atomicMin), so L[v] <= v at all times and a component's root is its smallest flat index: the first voxel in
// raster order, which is how scipy numbers components -- the tie rule of argmax(bincount) falls out of the key below.
// Every loop walks strictly decreasing labels (find: L[x] < x; union: max(a, b) decreases per round), so it ends whatever
// the scheduling; no thread ever waits for another thread's store.  Kernel boundaries are the only phase barriers.
//
//   cc_tile      one block per 8 x 8 x 32 tile: union-find inside LDS over the backward half of the neighbourhood (3 of 6,
//                13 of 26 neighbours), flattened, written as global flat indices (-1 on voxels that join nothing: class 0
//                and values >= C); cnt[v] = voxels of the tile under v where v is a tile-local root, else 0 (counted in
//                LDS, one atomic per run of equal roots in a wave).                      reads 1 B, writes 8 B per voxel
//   cc_border    voxels on tile faces unite with their backward neighbours in OTHER tiles: global atomicMin on the faces
//                only; the voxel's and its tile root's pointers are shortened to the root they found (atomicMin too).
//   cc_count     L[v] <- root(v) (the tile root's pointer is shortened for the next reader); a tile-local root that is not
//                the component's root adds its tile's count to cnt[root]: one global atomic per (tile, component), not
//                per voxel.                                                              reads 8 B, writes <= 4 B per voxel
//   cc_select    every root (L[v] == v) feeds its class: #components, #voxels and a 64-bit max of (size << 32 |
//                0xFFFFFFFF - root) -- largest first, smallest flat index among equals -- reduced in LDS per block, then
//                one atomic per class and block into the stats rows (used as scratch).   reads 4 B (+ 5 B per root)
//   cc_finalize  stats rows -> {components, kept, first voxel, removed}
//   cc_filter    out[v] = lab[v] unless v's class is a foreground class and L[v] is not the kept root.
//                                                                                        reads 5 B, writes 1 B per voxel
// HBM / atomic bound; nothing here is MFMA-shaped.
#include "common.h"

namespace {

constexpr int CC_TZ = 8, CC_TY = 8, CC_TX = 32, CC_TILE = CC_TZ * CC_TY * CC_TX;   // 2048 voxels, 8 per thread

struct LdsMem {
    static MSSEG_DEVFN int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static MSSEG_DEVFN int amin(int* p, int v) {
        return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
struct GlobalMem {
    static MSSEG_DEVFN int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static MSSEG_DEVFN int amin(int* p, int v) {
        return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// L[x] <= x everywhere: the walk strictly decreases until it stands on a root
template <class M> MSSEG_DEVFN int uf_find(const int* L, int x) {
    int p;
    while ((p = M::ld(L + x)) != x) x = p;
    return x;
}

// Unite the sets of a and b.  atomicMin(&L[a], b) with a > b both roots: if it returns a, a was still a root and now hangs
// under b.  Otherwise another thread moved L[a] to `old` < a in between; L[a] = min(old, b) keeps a below both, and the
// link a -> old that may have been replaced is restored by uniting old with b.  max(a, b) strictly decreases per round.
template <class M> MSSEG_DEVFN void uf_union(int* L, int a, int b) {
    for (;;) {
        a = uf_find<M>(L, a);
        b = uf_find<M>(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = M::amin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// (dz, dy, dx) precedes (0, 0, 0) in raster order and belongs to the neighbourhood
template <int CONN> MSSEG_DEVFN constexpr bool cc_backward(int dz, int dy, int dx) {
    const bool before = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
    const int n = (dz != 0) + (dy != 0) + (dx != 0);
    return before && (CONN == 26 || n == 1);
}

template <int CONN>
__global__ __launch_bounds__(256) void cc_tile_kernel(const unsigned char* lab, int D, int H, int W, int C, int tiles_y,
                                                      int tiles_x, int* __restrict__ L, int* __restrict__ cnt) {
    __shared__ int s_l[CC_TILE];
    __shared__ unsigned char s_c[CC_TILE];
    __shared__ int s_n[CC_TILE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, tz = blockIdx.x / (tiles_x * tiles_y);
    const int z0 = tz * CC_TZ, y0 = ty * CC_TY, x0 = tx * CC_TX;
#pragma unroll
    for (int k = 0; k < CC_TILE / 256; ++k) {
        const int li = tid + 256 * k;
        const int x = x0 + (li & 31), y = y0 + ((li >> 5) & 7), z = z0 + (li >> 8);
        unsigned char c = 0;
        if (x < W && y < H && z < D) c = lab[((long long)z * H + y) * W + x];
        s_c[li] = c < C ? c : (unsigned char)0;      // outside the volume and ignore labels: background, join nothing
        s_l[li] = li;                                // tile-local raster index: ordered as the global flat index
        s_n[li] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_TILE / 256; ++k) {
        const int li = tid + 256 * k;
        const int lx = li & 31, ly = (li >> 5) & 7, lz = li >> 8;
        const unsigned char c = s_c[li];
        if (c == 0) continue;
        // when the x-1 voxel is of the same class, its thread unites it with every neighbour of ours at dx <= 0 (they are
        // its neighbours at dx <= +1, in this tile or, by cc_border, in the next); x-1 itself and dx = +1 remain
        const bool left = lx > 0 && s_c[li - 1] == c;
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_backward<CONN>(dz, dy, dx)) continue;
                    const bool is_left = dz == 0 && dy == 0 && dx == -1;
                    if (CONN == 26 && left && dx <= 0 && !is_left) continue;
                    const int nx = lx + dx, ny = ly + dy, nz = lz + dz;
                    if (nx < 0 || nx >= CC_TX || ny < 0 || ny >= CC_TY || nz < 0) continue;
                    const int ni = li + dz * (CC_TY * CC_TX) + dy * CC_TX + dx;
                    if (s_c[ni] == c) uf_union<LdsMem>(s_l, li, ni);
                }
    }
    __syncthreads();
    int root[CC_TILE / 256];
#pragma unroll
    for (int k = 0; k < CC_TILE / 256; ++k) {
        const int li = tid + 256 * k;
        root[k] = s_c[li] ? uf_find<LdsMem>(s_l, li) : -1;
        // voxels per root: a wave holds 64 consecutive tile voxels; one LDS atomic per run of equal roots.  Every lane
        // of the block is here (no early exit above), so the shuffle and the ballot see whole waves.
        const int prev = __shfl_up(root[k], 1);
        const bool head = lane == 0 || prev != root[k];
        const unsigned long long heads = __ballot(head);
        if (head && root[k] >= 0) {
            const unsigned long long rest = (heads >> lane) >> 1;      // heads after this lane
            atomicAdd(s_n + root[k], rest ? __ffsll((long long)rest) : 64 - lane);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_TILE / 256; ++k) {
        const int li = tid + 256 * k;
        const int x = x0 + (li & 31), y = y0 + ((li >> 5) & 7), z = z0 + (li >> 8);
        if (x >= W || y >= H || z >= D) continue;
        const int g = (z * H + y) * W + x;           // D * H * W < 2^31
        const int r = root[k];
        L[g] = r < 0 ? -1 : ((z0 + (r >> 8)) * H + y0 + ((r >> 5) & 7)) * W + x0 + (r & 31);
        cnt[g] = s_n[li];
    }
}

// root of v; v's pointer and the pointer of the node it pointed to (its tile root) are shortened to that root.  atomicMin,
// because either may be a root that another thread hangs elsewhere at the same moment: a store could undo that link.
MSSEG_DEVFN int cc_find_shorten(int* L, int v) {
    const int p = GlobalMem::ld(L + v);
    if (p == v) return v;
    const int q = GlobalMem::ld(L + p);
    if (q == p) return p;
    const int r = uf_find<GlobalMem>(L, q);
    GlobalMem::amin(L + v, r);
    if (r != q) GlobalMem::amin(L + p, r);      // a tile's face voxels share p: only while its pointer is still long
    return r;
}

template <int CONN>
__global__ __launch_bounds__(256) void cc_border_kernel(const unsigned char* lab, int D, int H, int W, int C, int* L) {
    const int V = D * H * W;
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        const int x = i % W, y = (i / W) % H, z = i / (W * H);
        const int fx = x & (CC_TX - 1), fy = y & (CC_TY - 1), fz = z & (CC_TZ - 1);
        // a backward neighbour lies in another tile only from a low face or, at 26, from a high y / x face
        const bool face = fz == 0 || fy == 0 || fx == 0 || (CONN == 26 && (fy == CC_TY - 1 || fx == CC_TX - 1));
        if (!face) continue;
        const unsigned char c = lab[i];
        if (c == 0 || c >= C) continue;
        const bool left = x > 0 && lab[i - 1] == c;      // see cc_tile_kernel
        int ra = -1;
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_backward<CONN>(dz, dy, dx)) continue;
                    const bool is_left = dz == 0 && dy == 0 && dx == -1;
                    if (CONN == 26 && left && dx <= 0 && !is_left) continue;
                    const int nx = x + dx, ny = y + dy, nz = z + dz;
                    if (nx < 0 || nx >= W || ny < 0 || ny >= H || nz < 0) continue;
                    // same tile: done in LDS
                    if ((nx ^ x) < CC_TX && (ny ^ y) < CC_TY && (nz ^ z) < CC_TZ) continue;
                    const int ni = i + (dz * H + dy) * W + dx;
                    if (lab[ni] != c) continue;
                    if (ra < 0) ra = cc_find_shorten(L, i);
                    uf_union<GlobalMem>(L, ra, cc_find_shorten(L, ni));
                }
    }
}

__global__ __launch_bounds__(256) void cc_count_kernel(int V, int* L, int* cnt) {
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        const int p = GlobalMem::ld(L + i);
        if (p < 0) continue;
        const int r = uf_find<GlobalMem>(L, p);
        // no union runs in this kernel, so the roots are final and a store of an ancestor only shortens a path
        if (r != p) {
            __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (GlobalMem::ld(L + p) != r) __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // cnt[i] > 0 marks a tile-local root.  Sums arrive at component roots only, and a component root never gives, so
        // the plain read of cnt[i] never meets an atomic on the same word.
        const int n = cnt[i];
        if (n > 0 && r != i) atomicAdd(cnt + r, n);
    }
}

__global__ __launch_bounds__(256) void cc_select_kernel(const unsigned char* lab, int V, int C, const int* __restrict__ L,
                                                        const int* __restrict__ cnt, int* stats) {
    __shared__ int s_n[64], s_tot[64];
    __shared__ unsigned long long s_best[64];
    if (threadIdx.x < 64) { s_n[threadIdx.x] = 0; s_tot[threadIdx.x] = 0; s_best[threadIdx.x] = 0ull; }
    __syncthreads();
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        if (L[i] != i) continue;
        const int c = lab[i], n = cnt[i];                 // a root is a foreground voxel: 1 <= c < C <= 64
        atomicAdd(s_n + c, 1);
        atomicAdd(s_tot + c, n);
        atomicMax(s_best + c, ((unsigned long long)(unsigned)n << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < C && s_n[c] > 0) {
        atomicAdd(stats + 4 * c + 0, s_n[c]);
        atomicAdd(stats + 4 * c + 1, s_tot[c]);
        atomicMax((unsigned long long*)(stats + 4 * c + 2), s_best[c]);
    }
}

__global__ void cc_finalize_kernel(int C, int* stats) {
    const int c = threadIdx.x;
    if (c >= C) return;
    const int n = stats[4 * c + 0], tot = stats[4 * c + 1];
    const unsigned long long best = *(const unsigned long long*)(stats + 4 * c + 2);
    const int kept = (int)(best >> 32), first = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
    const bool any = c > 0 && n > 0;
    stats[4 * c + 0] = any ? n : 0;
    stats[4 * c + 1] = any ? kept : 0;
    stats[4 * c + 2] = any ? first : -1;
    stats[4 * c + 3] = any ? tot - kept : 0;
}

// lab and out may be the same buffer: every thread reads and writes its own voxel only
__global__ __launch_bounds__(256) void cc_filter_kernel(const unsigned char* lab, int V, int C, const int* __restrict__ L,
                                                        const int* __restrict__ stats, unsigned char* out) {
    __shared__ int s_keep[64];
    if (threadIdx.x < 64) s_keep[threadIdx.x] = threadIdx.x < C ? stats[4 * threadIdx.x + 2] : -1;
    __syncthreads();
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        const unsigned char c = lab[i];
        out[i] = (c >= 1 && c < C && L[i] != s_keep[c]) ? (unsigned char)0 : c;
    }
}

inline unsigned cc_grid(long long n, int per) {
    long long g = ceil_div_ll(n, per);
    const long long cap = (long long)msseg_num_cus() * 16;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int msseg_keep_largest_u8(const uint8_t* lab, int D, int H, int W, int n_classes, int connectivity, int32_t* work,
                                     int32_t* stats, uint8_t* out, msseg_stream_t stream) {
    if (!lab || !work || !stats || !out) MSSEG_FAIL(MSSEG_EINVAL, "keep_largest_u8: null pointer");
    if (connectivity != 6 && connectivity != 26)
        MSSEG_FAIL(MSSEG_EINVAL, "keep_largest_u8: connectivity %d (6 or 26)", connectivity);
    if (n_classes < 2 || n_classes > 64) MSSEG_FAIL(MSSEG_EINVAL, "keep_largest_u8: %d classes (2..64)", n_classes);
    if (D < 1 || H < 1 || W < 1) MSSEG_FAIL(MSSEG_EINVAL, "keep_largest_u8: empty volume %dx%dx%d", D, H, W);
    const long long V = (long long)D * H * W;
    if (V >= (1LL << 31)) MSSEG_FAIL(MSSEG_EINVAL, "keep_largest_u8: %dx%dx%d voxels do not fit int32 labels", D, H, W);
    if (((uintptr_t)stats & 7) || ((uintptr_t)work & 3))
        MSSEG_FAIL(MSSEG_EINVAL, "keep_largest_u8: stats must be 8-byte aligned, work 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int* L = work;
    int* cnt = work + V;
    const int tiles_z = ceil_div(D, CC_TZ), tiles_y = ceil_div(H, CC_TY), tiles_x = ceil_div(W, CC_TX);
    const long long tiles = (long long)tiles_z * tiles_y * tiles_x;       // <= D * H * W < 2^31: fits a grid
    if (hipMemsetAsync(stats, 0, (size_t)n_classes * 4 * sizeof(int32_t), s) != hipSuccess)
        MSSEG_FAIL(MSSEG_ELAUNCH, "keep_largest_u8: memset failed");
    if (connectivity == 6) {
        hipLaunchKernelGGL(cc_tile_kernel<6>, dim3((unsigned)tiles), dim3(256), 0, s, lab, D, H, W, n_classes, tiles_y, tiles_x,
                           L, cnt);
        hipLaunchKernelGGL(cc_border_kernel<6>, dim3(cc_grid(V, 256)), dim3(256), 0, s, lab, D, H, W, n_classes, L);
    } else {
        hipLaunchKernelGGL(cc_tile_kernel<26>, dim3((unsigned)tiles), dim3(256), 0, s, lab, D, H, W, n_classes, tiles_y, tiles_x,
                           L, cnt);
        hipLaunchKernelGGL(cc_border_kernel<26>, dim3(cc_grid(V, 256)), dim3(256), 0, s, lab, D, H, W, n_classes, L);
    }
    hipLaunchKernelGGL(cc_count_kernel, dim3(cc_grid(V, 256)), dim3(256), 0, s, (int)V, L, cnt);
    hipLaunchKernelGGL(cc_select_kernel, dim3(cc_grid(V, 256)), dim3(256), 0, s, lab, (int)V, n_classes, L, cnt, stats);
    hipLaunchKernelGGL(cc_finalize_kernel, dim3(1), dim3(64), 0, s, n_classes, stats);
    hipLaunchKernelGGL(cc_filter_kernel, dim3(cc_grid(V, 256)), dim3(256), 0, s, lab, (int)V, n_classes, L, stats, out);
    MSSEG_CHECK_LAUNCH("keep_largest_u8");
    return MSSEG_OK;
}
