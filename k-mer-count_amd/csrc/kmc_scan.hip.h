// kmc_scan.hip.h -- exclusive scan of a u32 sequence, three small kernels (block sums, scan of the sums, final) and the
// host function that launches them.  MODE 0: the values themselves; MODE 1: popcount of 64-bit words (bitmap rank)
#pragma once
#include "kmc_device.hip.h"

#define KMC_SCAN_PER_BLOCK 2048
template <int MODE>
__device__ __forceinline__ u32 scan_value(const void* src, u32 i) {
    if (MODE == 0) return reinterpret_cast<const u32*>(src)[i];
    return (u32)__popcll(reinterpret_cast<const unsigned long long*>(src)[i]);
}
template <int MODE>
__global__ __launch_bounds__(256)
void kmc_scan_sums_kernel(const void* __restrict__ src, u32 n, u32* __restrict__ bsum) {
    __shared__ u32 ws[4];
    const u32 tid = threadIdx.x, i0 = blockIdx.x * KMC_SCAN_PER_BLOCK + tid * 8;
    u32 s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) if (i0 + e < n) s += scan_value<MODE>(src, i0 + e);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) ws[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) bsum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
// in-place exclusive scan of up to a few hundred thousand block sums; total -> *total (one workgroup).  Not a template:
// defined in the one translation unit that asks for it (kmc_api.hip), declared for the other
__global__ __launch_bounds__(1024) void kmc_scan_top_kernel(u32* __restrict__ bsum, u32 nb, u32* __restrict__ total);
#ifdef KMC_SCAN_TOP_DEFINE
__global__ __launch_bounds__(1024) void kmc_scan_top_kernel(u32* __restrict__ bsum, u32 nb, u32* __restrict__ total) {
    __shared__ u32 part[1024];
    const u32 tid = threadIdx.x;
    const u32 per = (nb + 1023) / 1024;
    const u32 a = min(tid * per, nb), b = min(a + per, nb);
    u32 s = 0;
    for (u32 i = a; i < b; ++i) s += bsum[i];
    part[tid] = s;
    __syncthreads();
    for (u32 o = 1; o < 1024; o <<= 1) {
        u32 v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u32 run = tid ? part[tid - 1] : 0;
    for (u32 i = a; i < b; ++i) { const u32 v = bsum[i]; bsum[i] = run; run += v; }
    if (tid == 1023) *total = part[1023];
}
#endif
template <int MODE>
__global__ __launch_bounds__(256)
void kmc_scan_final_kernel(const void* __restrict__ src, u32 n, const u32* __restrict__ bbase, u32* __restrict__ out) {
    __shared__ u32 ws[4];
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i0 = blockIdx.x * KMC_SCAN_PER_BLOCK + tid * 8;
    u32 v[8], s = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = (i0 + e < n) ? scan_value<MODE>(src, i0 + e) : 0u; s += v[e]; }
    u32 inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(inc, o); if ((int)lane >= o) inc += t; }
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    u32 run = bbase[blockIdx.x] + inc - s;
    for (u32 w = 0; w < wv; ++w) run += ws[w];
#pragma unroll
    for (int e = 0; e < 8; ++e) { if (i0 + e < n) out[i0 + e] = run; run += v[e]; }
}

// out[i] = src[0] + ... + src[i - 1] (MODE as above) for i < n, *total = the sum of all; bsum: n / KMC_SCAN_PER_BLOCK + 2
// words of scratch.  Three launches on `stream`, nothing waited for (the caller checks hipGetLastError).
template <int MODE>
static inline void launch_exclusive_scan(hipStream_t stream, const void* src, u32 n, u32* bsum, u32* out, u32* total) {
    const u32 nb = (u32)(((u64)n + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK);
    hipLaunchKernelGGL(kmc_scan_sums_kernel<MODE>, dim3(nb), dim3(256), 0, stream, src, n, bsum);
    hipLaunchKernelGGL(kmc_scan_top_kernel, dim3(1), dim3(1024), 0, stream, bsum, nb, total);
    hipLaunchKernelGGL((kmc_scan_final_kernel<MODE>), dim3(nb), dim3(256), 0, stream, src, n, (const u32*)bsum, out);
}
