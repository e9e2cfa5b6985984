// Weight packing: torch-layout fp32 weights -> the images the MFMA kernels read, one image per launch or a whole
// network's images in one launch.
#include "common.h"

namespace {

template <typename T>
__global__ void pack_weights_kernel(const float* __restrict__ src, T* __restrict__ dst, int M, int M0, int Tt, int K,
                                    int K0, long long s_m1, long long s_m0, long long s_t, long long s_k1,
                                    long long s_k0, int flip, int coutb, int nkb, long long total) {
    constexpr int EPC = DT<T>::EPC;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long t = i;
        const int e = (int)(t % EPC); t /= EPC;
        const int col = (int)(t % coutb); t /= coutb;
        const int q = (int)(t % 4); t /= 4;
        const int tap = (int)(t % Tt); t /= Tt;
        const int kb = (int)(t % nkb);
        const int cb = (int)(t / nkb);
        const int m = cb * coutb + col;
        const int k = kb * 4 * EPC + q * EPC + e;
        float v = 0.f;
        if (m < M && k < K) {
            const int tt = flip ? (Tt - 1 - tap) : tap;
            v = src[(long long)(m / M0) * s_m1 + (long long)(m % M0) * s_m0 + (long long)tt * s_t +
                    (long long)(k / K0) * s_k1 + (long long)(k % K0) * s_k0];
        }
        DT<T>::st(dst + i, v);
    }
}

// All images of a network in one launch.  Flat grid: block b belongs to the job whose run of ceil(chunks / PACK_CPB) blocks
// contains b (the first wave finds it with a prefix sum over the table), so a table of many small and a few large images
// fills the chip evenly (a grid of [blocks of the largest image] x [jobs] left most blocks empty and the largest image on ~100 of
// them: 56 us for the UNet's 23 MB, 0.8 TB/s).  One thread packs PACK_CPT 16-byte chunks, all their source loads in flight together.
constexpr unsigned PACK_CPT = 4, PACK_CPB = 256 * PACK_CPT;

template <typename T>
__global__ __launch_bounds__(256) void pack_weights_batch_kernel(const msseg_pack_job* __restrict__ jobs, int njobs) {
    constexpr unsigned EPC = DT<T>::EPC;
    __shared__ int sel[2];
    if (threadIdx.x < 64) {
        const unsigned lane = threadIdx.x;
        if (lane == 0) sel[0] = -1;
        unsigned before = 0;
        for (int base = 0; base < njobs; base += 64) {   // wave-uniform trip count and exit
            const int jj = base + (int)lane;
            const unsigned nb = jj < njobs ? (unsigned)((jobs[jj].total / EPC + PACK_CPB - 1) / PACK_CPB) : 0u;
            unsigned incl = nb;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_up(incl, o);
                if ((int)lane >= o) incl += v;
            }
            const unsigned lo = before + incl - nb;
            const bool mine = blockIdx.x >= lo && blockIdx.x < lo + nb;
            if (mine) { sel[0] = jj; sel[1] = (int)(blockIdx.x - lo); }
            if (__ballot(mine)) break;
            before += __shfl(incl, 63);
        }
    }
    __syncthreads();
    if (sel[0] < 0) return;            // a block past the last job's run (the host rounds the grid up)
    const msseg_pack_job j = jobs[sel[0]];
    T* dst = (T*)j.dst;
    // 32-bit index arithmetic (images are far below 2^31 elements)
    const unsigned nchunks = (unsigned)(j.total / EPC), cb_w = (unsigned)j.cout_block, Tt = (unsigned)j.T, nkb = (unsigned)j.nkb;
    // work order: eight neighbouring columns fastest (eight lanes fill one 128-byte line of the image), then the taps (neighbouring
    // source elements of a conv weight, [m][k][tap] in torch layout), then the other columns; the destination chunk index is
    // recomputed from the coordinates
    const unsigned cb8 = cb_w >> 3;
    float v[PACK_CPT][EPC];
    unsigned ch[PACK_CPT];
#pragma unroll
    for (unsigned i = 0; i < PACK_CPT; ++i) {
        const unsigned wi = (unsigned)sel[1] * PACK_CPB + i * 256u + threadIdx.x;
        ch[i] = 0xffffffffu;
#pragma unroll
        for (unsigned e = 0; e < EPC; ++e) v[i][e] = 0.f;
        if (wi >= nchunks) continue;
        unsigned t = wi;
        const unsigned col_lo = t & 7u; t >>= 3;
        const unsigned tap = t % Tt; t /= Tt;
        const unsigned col = (t % cb8) * 8u + col_lo; t /= cb8;
        const unsigned q = t & 3u; t >>= 2;
        const unsigned kb = t % nkb;
        const unsigned cb = t / nkb;
        ch[i] = (((cb * nkb + kb) * Tt + tap) * 4u + q) * cb_w + col;
        const int m = (int)(cb * cb_w + col);
        if (m >= j.M) continue;
        const unsigned tt = j.flip ? (Tt - 1 - tap) : tap;
        const long long mbase = (long long)(m / j.M0) * j.s_m1 + (long long)(m % j.M0) * j.s_m0 + (long long)tt * j.s_t;
        // k = k1 * K0 + k0 of the chunk's first element by one division, the other seven by carry (16 runtime divisions per chunk
        // made this pass instruction-bound)
        const int kfirst = (int)(kb * 4 * EPC + q * EPC);
        int k1 = kfirst / j.K0, k0 = kfirst - k1 * j.K0;
#pragma unroll
        for (unsigned e = 0; e < EPC; ++e) {
            if (kfirst + (int)e < j.K) v[i][e] = j.src[mbase + (long long)k1 * j.s_k1 + (long long)k0 * j.s_k0];
            if (++k0 == j.K0) { k0 = 0; ++k1; }
        }
    }
#pragma unroll
    for (unsigned i = 0; i < PACK_CPT; ++i) {
        if (ch[i] == 0xffffffffu) continue;
        alignas(16) T out[EPC];
#pragma unroll
        for (unsigned e = 0; e < EPC; ++e) DT<T>::st(&out[e], v[i][e]);
        *(u32x4_t*)(dst + (size_t)ch[i] * EPC) = *(const u32x4_t*)out;
    }
}

}  // namespace

extern "C" {

size_t msseg_packed_weight_bytes(int M, int T, int K, int cout_block, int dtype) {
    const int epc = epc_of(dtype);
    const size_t ncb = (size_t)ceil_div(M, cout_block), nkb = (size_t)ceil_div(K, 4 * epc);
    return ncb * nkb * (size_t)T * 4 * (size_t)cout_block * 16;
}

int msseg_pack_weights(const float* src, void* dst, int dtype, int M, int M0, int T, int K, int K0, long long s_m1,
                       long long s_m0, long long s_t, long long s_k1, long long s_k0, int flip, int cout_block,
                       msseg_stream_t stream) {
    if (!src || !dst || M < 1 || T < 1 || K < 1 || M0 < 1 || K0 < 1) MSSEG_FAIL(MSSEG_EINVAL, "pack_weights: bad args");
    if (cout_block != 16 && cout_block != 32 && cout_block != 48) MSSEG_FAIL(MSSEG_EINVAL, "pack_weights: bad cout block");
    const int esz = dtype == MSSEG_F32 ? 4 : 2;
    const long long total = (long long)(msseg_packed_weight_bytes(M, T, K, cout_block, dtype) / esz);
    const int nkb = ceil_div(K, 64 / esz);
    const bool known = for_dtype(dtype, [&](auto t) {
        using TD = typename decltype(t)::type;
        hipLaunchKernelGGL(pack_weights_kernel<TD>, dim3(stream_grid(total, 1024)), dim3(256), 0, (hipStream_t)stream, src,
                           (TD*)dst, M, M0, T, K, K0, s_m1, s_m0, s_t, s_k1, s_k0, flip, cout_block, nkb, total);
    });
    if (!known) return bad_dtype(dtype);
    MSSEG_CHECK_LAUNCH("pack_weights");
    return MSSEG_OK;
}

int msseg_pack_weights_batch(const msseg_pack_job* jobs_dev, int njobs, long long max_total, long long sum_total, int dtype,
                             msseg_stream_t stream) {
    if (!jobs_dev || njobs < 1 || njobs > 65535 || max_total < 1 || sum_total < max_total)
        MSSEG_FAIL(MSSEG_EINVAL, "pack_weights_batch: bad args");
    const long long epc = epc_of(dtype);
    if (max_total / epc >= 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "pack_weights_batch: image too large");
    // sum over the jobs of ceil(chunks / PACK_CPB) <= sum of chunks / PACK_CPB + njobs: the blocks past the end find no job and exit
    const long long gx = sum_total / epc / PACK_CPB + njobs + 1;
    if (gx >= 0x7fffffffLL) MSSEG_FAIL(MSSEG_EINVAL, "pack_weights_batch: too many blocks");
    dim3 grid((unsigned)gx);
    const bool known = for_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(pack_weights_batch_kernel<typename decltype(t)::type>, grid, dim3(256), 0, (hipStream_t)stream, jobs_dev,
                           njobs);
    });
    if (!known) return bad_dtype(dtype);
    MSSEG_CHECK_LAUNCH("pack_weights_batch");
    return MSSEG_OK;
}

}  // extern "C"
