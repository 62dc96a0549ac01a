// kmc_partition.hip.h -- the sorted view cut into owner parts for the multi-GPU all-to-all (kmc_partition_device): count
// the pairs of every owner, then scatter them to the owners' spans.  Read by the view layer alone (kmc_views.hip).
#pragma once
#include "kmc_device.hip.h"

// part_cnt[p] = pairs whose owner is p
__global__ void kmc_owner_count_kernel(const u64* __restrict__ hi, const u64* __restrict__ lo, u64 n, u32 n_parts, unsigned long long* __restrict__ part_cnt) {
    extern __shared__ unsigned int oc_smem[];
    for (u32 p = threadIdx.x; p < n_parts; p += blockDim.x) oc_smem[p] = 0;
    __syncthreads();
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) atomicAdd(&oc_smem[kmc_owner(hi ? hi[i] : 0ull, lo[i], n_parts)], 1u);
    __syncthreads();
    for (u32 p = threadIdx.x; p < n_parts; p += blockDim.x) if (oc_smem[p]) atomicAdd(&part_cnt[p], (unsigned long long)oc_smem[p]);
}
// pairs to their owner's span (cursor[p] starts at the span's begin); the order inside a span is
// arbitrary (the receiver merges pairs into its table).  One global add per (wave, owner present in it).
__global__ void kmc_owner_scatter_kernel(const u64* __restrict__ hi, const u64* __restrict__ lo, const u64* __restrict__ cnt, u64 n, u32 n_parts,
                                         unsigned long long* __restrict__ cursor, u64* __restrict__ o_hi, u64* __restrict__ o_lo, u64* __restrict__ o_cnt) {
    const u64 n_round = (n + 63) & ~63ull;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += (u64)gridDim.x * blockDim.x) {
        const bool in = i < n;
        const u32 mine = in ? kmc_owner(hi ? hi[i] : 0ull, lo[i], n_parts) : ~0u;
        bool todo = in;
        u64 pos = 0;
        unsigned long long pending;
        while ((pending = __builtin_amdgcn_ballot_w64(todo)) != 0) {
            const u32 p = (u32)__builtin_amdgcn_readlane((int)mine, (int)__builtin_ctzll(pending));
            const unsigned long long grp = __builtin_amdgcn_ballot_w64(todo && mine == p);
            unsigned long long base = 0;
            if ((threadIdx.x & 63) == (u32)__builtin_ctzll(grp)) base = atomicAdd(&cursor[p], (unsigned long long)__popcll(grp));
            base = ((unsigned long long)(u32)__builtin_amdgcn_readlane((int)(u32)(base >> 32), (int)__builtin_ctzll(grp)) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)base, (int)__builtin_ctzll(grp));
            if (todo && mine == p) {
                pos = base + __builtin_amdgcn_mbcnt_hi((u32)(grp >> 32), __builtin_amdgcn_mbcnt_lo((u32)grp, 0u));
                todo = false;
            }
        }
        if (in) {
            o_lo[pos] = lo[i];
            o_cnt[pos] = cnt[i];
            if (hi) o_hi[pos] = hi[i];
        }
    }
}
