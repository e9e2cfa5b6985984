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
//                13 of 26 neighbours), flattened, written as global flat indices (-1 on voxels that join nothing: key 0,
//                for the classes class 0 and values >= C); cnt[v] = voxels of the tile under v where v is a tile-local root, else 0 (counted in
//                LDS, one atomic per run of equal roots in a wave).                      reads 1 B, writes 8 B per voxel
//   cc_border    voxels on tile faces unite with their backward neighbours in OTHER tiles: global atomicMin on the faces
//                only; the voxel's and its tile root's pointers are shortened to the root they found (atomicMin too).
//                A pair whose pointers meet after one step each is in one set already: four loads, no atomic.
//   cc_count     L[v] <- root(v) (the tile root's pointer is shortened for the next reader); a tile-local root that is not
//                the component's root adds its tile's count to cnt[root]: one global atomic per (tile, component), not
//                per voxel.                                                              reads 8 B, writes <= 4 B per voxel
//   cc_select    every root (L[v] == v) feeds its class: #components, #voxels and a 64-bit max of (size << 32 |
//                0xFFFFFFFF - root) -- largest first, smallest flat index among equals -- reduced in LDS per block, then
//                one atomic per class and block into the stats rows (used as scratch).   reads 4 B (+ 5 B per root)
//   cc_filter    out[v] = lab[v] unless v's class is a foreground class and L[v] is not the kept root.
//                                                                                        reads 5 B, writes 1 B per voxel
//   cc_finalize  stats rows -> {components, kept, first voxel, removed}
// msseg_postprocess_u8 runs up to three clean-up steps in a fixed order on the same machinery:
//   1 remove small components (MONAI RemoveSmallObjects, nnU-Net) and 2 keep the largest share ONE labelling: cc_select also
//     counts the components and voxels below min_size, cc_filter drops a voxel whose root's size cnt[L[v]] is below min_size
//     or whose root is not the kept one (a 4 B gather per foreground voxel more, only when keep-largest is off).
//   3 fill holes (MONAI FillHoles, scipy binary_fill_holes), class by class in ascending order on the map the class before
//     left: cc_tile / cc_border label the COMPLEMENT of class c (every voxel != c takes part and all of them may unite:
//     cc_key below is the one predicate both uses share); no cc_count pass, the two passes below find the roots themselves
//   cc_face      the voxels of the six volume faces mark the root of their component: cnt[root] = -1 (a count is >= 1)
//                                                                      reads 5 B (+ the path to the root) per face voxel
//   cc_fill      map[v] = c where map[v] != c and the root of v is not marked; counts them.
//                                                          reads 5 B (+ the path to the root), writes <= 1 B per voxel
//   cc_hist      voxels per foreground class of the final map (one LDS atomic per run of equal values in a wave); only
//                after a fill step or when the classes were not labelled: otherwise the counts follow from cc_select's
//                sums.                                                                   reads 1 B per voxel
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

// Which voxels take part and which neighbours may unite: voxels unite when their keys are equal and not 0.
//   fc == 0  the classes: a foreground class is its own key; class 0 and values >= C join nothing
//   fc >= 1  the complement of class fc: every voxel that is not fc has key 1 (values >= C too: a leak path may cross them)
MSSEG_DEVFN unsigned char cc_key(unsigned char c, int C, int fc) {
    if (fc) return (unsigned char)(c != fc);
    return c < C ? c : (unsigned char)0;
}

template <int CONN>
__global__ __launch_bounds__(256) void cc_tile_kernel(const unsigned char* lab, int D, int H, int W, int C, int fc, int tiles_y,
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
        unsigned char c = 0;                         // outside the volume: joins nothing
        if (x < W && y < H && z < D) c = cc_key(lab[((long long)z * H + y) * W + x], C, fc);
        s_c[li] = c;
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
        // when the x-1 voxel has the same key, its thread unites it with every neighbour of ours at dx <= 0 (they are
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
__global__ __launch_bounds__(256) void cc_border_kernel(const unsigned char* lab, int D, int H, int W, int C, int fc, int* L) {
    const int V = D * H * W;
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        const int x = i % W, y = (i / W) % H, z = i / (W * H);
        const int fx = x & (CC_TX - 1), fy = y & (CC_TY - 1), fz = z & (CC_TZ - 1);
        // a backward neighbour lies in another tile only from a low face or, at 26, from a high y / x face
        const bool face = fz == 0 || fy == 0 || fx == 0 || (CONN == 26 && (fy == CC_TY - 1 || fx == CC_TX - 1));
        if (!face) continue;
        const unsigned char c = cc_key(lab[i], C, fc);
        if (c == 0) continue;
        const bool left = x > 0 && cc_key(lab[i - 1], C, fc) == c;      // see cc_tile_kernel
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
                    if (cc_key(lab[ni], C, fc) != c) continue;
                    // One step up from each side's pointer: the same node means one set already.  On the faces of a
                    // solid region every voxel pair repeats the union of the same two tile roots; after the first one
                    // the rest leave here with four loads and no atomic.  (Both pointers are >= 0: the keys are not 0.)
                    if (GlobalMem::ld(L + GlobalMem::ld(L + i)) == GlobalMem::ld(L + GlobalMem::ld(L + ni))) continue;
                    if (ra < 0) ra = cc_find_shorten(L, i);
                    uf_union<GlobalMem>(L, ra, cc_find_shorten(L, ni));
                }
    }
}

// Root of the node p once every union is done (a kernel after cc_border): the roots are final, so a store of an ancestor
// only shortens a path.  p's pointer is shortened for the next reader: a tile's voxels share their tile root p.
MSSEG_DEVFN int cc_final_root(int* L, int p) {
    const int r = uf_find<GlobalMem>(L, p);
    if (r != p && GlobalMem::ld(L + p) != r) __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return r;
}

__global__ __launch_bounds__(256) void cc_count_kernel(int V, int* L, int* cnt) {
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        const int p = GlobalMem::ld(L + i);
        if (p < 0) continue;
        const int r = cc_final_root(L, p);
        if (r != p) __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // cnt[i] > 0 marks a tile-local root.  Sums arrive at component roots only, and a component root never gives, so
        // the plain read of cnt[i] never meets an atomic on the same word.
        const int n = cnt[i];
        if (n > 0 && r != i) atomicAdd(cnt + r, n);
    }
}

// Raw rows of `stats` while the passes run, S ints per class (S = 4: keep_largest_u8, S = 6: postprocess_u8):
// {components, voxels, 64-bit best key in [2] and [3], components below min_size, voxels in them}; the last two only at S = 6.
__global__ __launch_bounds__(256) void cc_select_kernel(const unsigned char* lab, int V, int C, const int* __restrict__ L,
                                                        const int* __restrict__ cnt, int min_size, int S, int* stats) {
    __shared__ int s_n[64], s_tot[64], s_sn[64], s_stot[64];
    __shared__ unsigned long long s_best[64];
    if (threadIdx.x < 64) {
        s_n[threadIdx.x] = 0; s_tot[threadIdx.x] = 0; s_sn[threadIdx.x] = 0; s_stot[threadIdx.x] = 0;
        s_best[threadIdx.x] = 0ull;
    }
    __syncthreads();
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        if (L[i] != i) continue;
        const int c = lab[i], n = cnt[i];                 // a root is a foreground voxel: 1 <= c < C <= 64
        atomicAdd(s_n + c, 1);
        atomicAdd(s_tot + c, n);
        atomicMax(s_best + c, ((unsigned long long)(unsigned)n << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i));
        if (n < min_size) { atomicAdd(s_sn + c, 1); atomicAdd(s_stot + c, n); }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < C && s_n[c] > 0) {
        atomicAdd(stats + S * c + 0, s_n[c]);
        atomicAdd(stats + S * c + 1, s_tot[c]);
        atomicMax((unsigned long long*)(stats + S * c + 2), s_best[c]);
        if (s_sn[c] > 0) {                                // min_size > 1 comes with S = 6 only
            atomicAdd(stats + S * c + 4, s_sn[c]);
            atomicAdd(stats + S * c + 5, s_stot[c]);
        }
    }
}

MSSEG_DEVFN int cc_best_size(unsigned long long best) { return (int)(best >> 32); }
MSSEG_DEVFN int cc_best_root(unsigned long long best) { return (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)); }

// A foreground voxel is dropped when its component is not the kept one (keep_largest; a largest component below min_size
// keeps nothing) or, without keep_largest, when its component holds fewer than min_size voxels.  Reads the raw rows.
// lab and out may be the same buffer: every thread reads and writes its own voxel only
__global__ __launch_bounds__(256) void cc_filter_kernel(const unsigned char* lab, int V, int C, const int* __restrict__ L,
                                                        const int* __restrict__ cnt, int min_size, int keep_largest, int S,
                                                        const int* __restrict__ stats, unsigned char* out) {
    __shared__ int s_keep[64];
    if (threadIdx.x < 64) {
        int keep = -1;
        if (threadIdx.x < C) {
            const unsigned long long best = *(const unsigned long long*)(stats + S * threadIdx.x + 2);
            if (cc_best_size(best) > 0 && cc_best_size(best) >= min_size) keep = cc_best_root(best);
        }
        s_keep[threadIdx.x] = keep;
    }
    __syncthreads();
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        const unsigned char c = lab[i];
        bool drop = false;
        if (c >= 1 && c < C) {
            const int r = L[i];
            drop = keep_largest ? r != s_keep[c] : cnt[r] < min_size;
        }
        out[i] = drop ? (unsigned char)0 : c;
    }
}

// raw rows -> {components, kept, first voxel, removed} of keep_largest_u8
__global__ void cc_finalize_kernel(int C, int* stats) {
    const int c = threadIdx.x;
    if (c >= C) return;
    const int n = stats[4 * c + 0], tot = stats[4 * c + 1];
    const unsigned long long best = *(const unsigned long long*)(stats + 4 * c + 2);
    const int kept = cc_best_size(best), first = cc_best_root(best);
    const bool any = c > 0 && n > 0;
    stats[4 * c + 0] = any ? n : 0;
    stats[4 * c + 1] = any ? kept : 0;
    stats[4 * c + 2] = any ? first : -1;
    stats[4 * c + 3] = any ? tot - kept : 0;
}

// raw rows -> {components (-1: the classes were not labelled), components removed as small, voxels removed as small, voxels
// removed by keep-largest, 0, voxels left} of postprocess_u8.  cc_fill adds to column 4 afterwards; column 5 is 0 when
// cc_hist is to count the final map instead (hist: a fill step follows, or the classes were not labelled).
__global__ void pp_finalize_kernel(int C, int labelled, int min_size, int keep_largest, int hist, int* stats) {
    const int c = threadIdx.x;
    if (c >= C) return;
    const int n = stats[6 * c + 0], tot = stats[6 * c + 1], small_n = stats[6 * c + 4], small_tot = stats[6 * c + 5];
    const int kept = cc_best_size(*(const unsigned long long*)(stats + 6 * c + 2));
    const bool fg = c > 0;
    const int removed = fg && keep_largest && kept >= min_size ? tot - small_tot - kept : 0;
    stats[6 * c + 0] = !fg ? 0 : labelled ? n : -1;
    stats[6 * c + 1] = fg ? small_n : 0;
    stats[6 * c + 2] = fg ? small_tot : 0;
    stats[6 * c + 3] = removed;
    stats[6 * c + 4] = 0;
    stats[6 * c + 5] = fg && !hist ? tot - small_tot - removed : 0;
}

// The voxels of the six faces of the volume (edges and corners come up more than once) mark the root of their component of
// the complement of class fc: it reaches the outside.  Runs right after cc_border: L[v] is v's tile root or a node nearer
// the root, cnt[root] still the root's count inside its own tile, >= 1; the mark is -1.  One component may own most of the
// faces: the mark is read first, so that its word is stored to a few times and not once per face voxel.
__global__ __launch_bounds__(256) void cc_face_kernel(const unsigned char* map, int D, int H, int W, int fc, int* L, int* cnt) {
    const long long fz = (long long)H * W, fy = (long long)D * W, fx = (long long)D * H, n = 2 * (fz + fy + fx);
    for (long long j = blockIdx.x * 256LL + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        int z, y, x;
        if (j < 2 * fz) {
            const int r = (int)(j % fz);
            z = j < fz ? 0 : D - 1; y = r / W; x = r % W;
        } else if (j < 2 * (fz + fy)) {
            const long long k = j - 2 * fz;
            const int r = (int)(k % fy);
            y = k < fy ? 0 : H - 1; z = r / W; x = r % W;
        } else {
            const long long k = j - 2 * (fz + fy);
            const int r = (int)(k % fx);
            x = k < fx ? 0 : W - 1; z = r / H; y = r % H;
        }
        const int v = (z * H + y) * W + x;               // 0 <= z < D, 0 <= y < H, 0 <= x < W: inside the volume
        if (map[v] == fc) continue;
        const int r = cc_final_root(L, GlobalMem::ld(L + v));      // L[v] >= 0 on every voxel that is not fc
        if (GlobalMem::ld(cnt + r) >= 0) __hip_atomic_store(cnt + r, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// map[v] = fc where v is not of class fc and the root of its component of the complement is not marked; *filled += their
// number.  Finds the root itself (two or three loads, the tile root's pointer is short after its first reader) instead of
// a cc_count pass that would write it to every voxel.
__global__ __launch_bounds__(256) void cc_fill_kernel(unsigned char* map, int V, int fc, int* L, const int* __restrict__ cnt,
                                                      int* filled) {
    __shared__ int s_fill;
    if (threadIdx.x == 0) s_fill = 0;
    __syncthreads();
    int n = 0;
    for (long long i64 = blockIdx.x * 256LL + threadIdx.x; i64 < V; i64 += (long long)gridDim.x * 256) {
        const int i = (int)i64;
        if (map[i] == fc) continue;
        if (cnt[cc_final_root(L, GlobalMem::ld(L + i))] < 0) continue;
        map[i] = (unsigned char)fc;
        ++n;
    }
    if (n) atomicAdd(&s_fill, n);
    __syncthreads();
    if (threadIdx.x == 0 && s_fill) atomicAdd(filled, s_fill);
}

// stats[S * c + col] += voxels of class c in map, c in 1..C-1.  A wave holds 64 consecutive voxels: one LDS atomic per run of
// equal values, as in cc_tile_kernel; the loop bound is the same for the whole block, so the shuffle and the ballot see whole
// waves.
__global__ __launch_bounds__(256) void cc_hist_kernel(const unsigned char* map, int V, int C, int S, int col, int* stats) {
    __shared__ int s_h[64];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) s_h[threadIdx.x] = 0;
    __syncthreads();
    for (long long base = blockIdx.x * 256LL; base < V; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        int c = i < V ? map[i] : 0;
        if (c >= C) c = 0;
        const int prev = __shfl_up(c, 1);
        const bool head = lane == 0 || prev != c;
        const unsigned long long heads = __ballot(head);
        if (head && c > 0) {
            const unsigned long long rest = (heads >> lane) >> 1;      // heads after this lane
            atomicAdd(s_h + c, rest ? __ffsll((long long)rest) : 64 - lane);
        }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c > 0 && c < C && s_h[c] > 0) atomicAdd(stats + S * c + col, s_h[c]);
}

// One labelling.  fc == 0: the components of every foreground class; afterwards L[v] is the root of v's component (-1 where
// v joins nothing) and cnt[root] its size.  fc >= 1: the components of the complement of class fc (cc_key), without the
// flatten + count pass: L[v] leads to the root (cc_final_root) and cnt[root] >= 1.
void cc_label(hipStream_t s, const unsigned char* map, int D, int H, int W, int C, int connectivity, int fc, int* L, int* cnt) {
    const long long V = (long long)D * H * W;
    const int tiles_z = ceil_div(D, CC_TZ), tiles_y = ceil_div(H, CC_TY), tiles_x = ceil_div(W, CC_TX);
    const long long tiles = (long long)tiles_z * tiles_y * tiles_x;       // <= D * H * W < 2^31: fits a grid
    if (connectivity == 6) {
        hipLaunchKernelGGL(cc_tile_kernel<6>, dim3((unsigned)tiles), dim3(256), 0, s, map, D, H, W, C, fc, tiles_y, tiles_x, L,
                           cnt);
        hipLaunchKernelGGL(cc_border_kernel<6>, dim3(stream_grid(V)), dim3(256), 0, s, map, D, H, W, C, fc, L);
    } else {
        hipLaunchKernelGGL(cc_tile_kernel<26>, dim3((unsigned)tiles), dim3(256), 0, s, map, D, H, W, C, fc, tiles_y, tiles_x, L,
                           cnt);
        hipLaunchKernelGGL(cc_border_kernel<26>, dim3(stream_grid(V)), dim3(256), 0, s, map, D, H, W, C, fc, L);
    }
    if (!fc) hipLaunchKernelGGL(cc_count_kernel, dim3(stream_grid(V)), dim3(256), 0, s, (int)V, L, cnt);
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
    if (hipMemsetAsync(stats, 0, (size_t)n_classes * 4 * sizeof(int32_t), s) != hipSuccess)
        MSSEG_FAIL(MSSEG_ELAUNCH, "keep_largest_u8: memset failed");
    cc_label(s, lab, D, H, W, n_classes, connectivity, 0, L, cnt);
    hipLaunchKernelGGL(cc_select_kernel, dim3(stream_grid(V)), dim3(256), 0, s, lab, (int)V, n_classes, L, cnt, 0, 4, stats);
    hipLaunchKernelGGL(cc_filter_kernel, dim3(stream_grid(V)), dim3(256), 0, s, lab, (int)V, n_classes, L, cnt, 0, 1, 4, stats,
                       out);
    hipLaunchKernelGGL(cc_finalize_kernel, dim3(1), dim3(64), 0, s, n_classes, stats);
    MSSEG_CHECK_LAUNCH("keep_largest_u8");
    return MSSEG_OK;
}

extern "C" int msseg_postprocess_u8(const uint8_t* lab, int D, int H, int W, int n_classes, int min_size, int keep_largest,
                                    int connectivity, int fill_holes, int hole_connectivity, int32_t* work, int32_t* stats,
                                    uint8_t* out, msseg_stream_t stream) {
    if (!lab || !work || !stats || !out) MSSEG_FAIL(MSSEG_EINVAL, "postprocess_u8: null pointer");
    if (connectivity != 6 && connectivity != 26)
        MSSEG_FAIL(MSSEG_EINVAL, "postprocess_u8: connectivity %d (6 or 26)", connectivity);
    if (hole_connectivity != 6 && hole_connectivity != 26)
        MSSEG_FAIL(MSSEG_EINVAL, "postprocess_u8: hole connectivity %d (6 or 26)", hole_connectivity);
    if (n_classes < 2 || n_classes > 64) MSSEG_FAIL(MSSEG_EINVAL, "postprocess_u8: %d classes (2..64)", n_classes);
    if (min_size < 0) MSSEG_FAIL(MSSEG_EINVAL, "postprocess_u8: min_size %d is negative", min_size);
    if (D < 1 || H < 1 || W < 1) MSSEG_FAIL(MSSEG_EINVAL, "postprocess_u8: empty volume %dx%dx%d", D, H, W);
    const long long V = (long long)D * H * W;
    if (V >= (1LL << 31)) MSSEG_FAIL(MSSEG_EINVAL, "postprocess_u8: %dx%dx%d voxels do not fit int32 labels", D, H, W);
    if (((uintptr_t)stats & 7) || ((uintptr_t)work & 3))
        MSSEG_FAIL(MSSEG_EINVAL, "postprocess_u8: stats must be 8-byte aligned, work 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int* L = work;
    int* cnt = work + V;
    const unsigned grid = stream_grid(V);
    const int labelled = min_size > 1 || keep_largest;
    const int hist = fill_holes || !labelled;      // else the final voxel counts follow from the labelling's own sums
    if (hipMemsetAsync(stats, 0, (size_t)n_classes * 6 * sizeof(int32_t), s) != hipSuccess)
        MSSEG_FAIL(MSSEG_ELAUNCH, "postprocess_u8: memset failed");
    if (labelled) {
        cc_label(s, lab, D, H, W, n_classes, connectivity, 0, L, cnt);
        hipLaunchKernelGGL(cc_select_kernel, dim3(grid), dim3(256), 0, s, lab, (int)V, n_classes, L, cnt, min_size, 6, stats);
        hipLaunchKernelGGL(cc_filter_kernel, dim3(grid), dim3(256), 0, s, lab, (int)V, n_classes, L, cnt, min_size,
                           keep_largest ? 1 : 0, 6, stats, out);
    } else if (out != lab) {
        if (hipMemcpyAsync(out, lab, (size_t)V, hipMemcpyDeviceToDevice, s) != hipSuccess)
            MSSEG_FAIL(MSSEG_ELAUNCH, "postprocess_u8: copy failed");
    }
    hipLaunchKernelGGL(pp_finalize_kernel, dim3(1), dim3(64), 0, s, n_classes, labelled, min_size, keep_largest ? 1 : 0, hist,
                       stats);
    if (fill_holes) {
        const long long faces = 2 * ((long long)H * W + (long long)D * W + (long long)D * H);
        for (int fc = 1; fc < n_classes; ++fc) {      // in ascending order, each class on the map the class before left
            cc_label(s, out, D, H, W, n_classes, hole_connectivity, fc, L, cnt);
            hipLaunchKernelGGL(cc_face_kernel, dim3(stream_grid(faces)), dim3(256), 0, s, out, D, H, W, fc, L, cnt);
            hipLaunchKernelGGL(cc_fill_kernel, dim3(grid), dim3(256), 0, s, out, (int)V, fc, L, cnt, stats + 6 * fc + 4);
        }
    }
    if (hist) hipLaunchKernelGGL(cc_hist_kernel, dim3(grid), dim3(256), 0, s, out, (int)V, n_classes, 6, 5, stats);
    MSSEG_CHECK_LAUNCH("postprocess_u8");
    return MSSEG_OK;
}
