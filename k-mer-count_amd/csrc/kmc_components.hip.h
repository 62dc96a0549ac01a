// kmc_components.hip.h -- the connected components of the compacted graph (include/kmc.h: kmc_unitig_components,
// kmc_unitig_components_device, kmc_unitig_components_into): a component number per unitig, four words per component
// (root, unitigs, keys, abundance), a verdict per unitig -- keep, or component when its component is small -- and the table
// of the keys of the kept unitigs.
//
// What a links call leaves on the device is all this needs: the unitig arrays (offsets, abund) and the link records
// (link_offsets per end, link_to); the kept table then goes through the mark and scatter kernels of kmc_clean.hip.h.
//   label     parent[u] = u, then rounds of two passes.  hook: a lane per unitig end, at most four records; for every
//             record both unitigs are chased to the roots of their trees and, where the roots differ, the larger root is
//             hooked under the smaller with atomicMin; a workgroup that hooked anything adds to the round's counter.
//             shortcut: a lane per unitig, parent[u] = the root of u's tree.
//             INVARIANT: parent[x] <= x always and a parent only ever decreases (atomicMin with a smaller id; a shortcut
//             writes an ancestor, which is smaller).  So the parents form a forest whose trees never leave a component,
//             a chase takes at most n_unitigs steps, and the root of a tree is its smallest id.  A read that is stale
//             inside a launch (another XCD's L2, this CU's L1) is an older parent: a larger ancestor, which changes which
//             two ids a lane hooks, never whether they belong together.
//             TERMINATION is a hook pass whose counter stayed 0: it issued no atomic, so the array did not change while
//             it ran, so every value it read was the one the launch boundary made visible, and it found every record
//             with both ends in one tree: the trees are the components.  Nothing here waits for another workgroup.
//             A root that a hook pass hooks was a root when the pass began and is none when it ends, so a pass with a
//             non-zero counter leaves at least one root fewer: n_unitigs passes at most (the host's hard cap).
//   number    flag the roots, scan the flags (kmc_scan.hip.h): a root's rank is its component's number, the total the
//             number of components; comp_of[u] = rank[parent[u]], comp_stats[c][0] = the root.
//   stats     a lane per unitig adds (1, m_u, A_u) to its component's words with 64-bit integer atomics: exact whatever
//             the order.  Lanes of a wave that share a component are summed first -- up to KMC_CC_LEADERS times the wave
//             takes the component of its first lane not yet served, sums the lanes that share it, and that one lane adds;
//             whoever is left adds for itself.  (One giant component and little else is what real graphs look like: then
//             a wave adds once or twice, not 64 times to one address.)
//   verdict   a lane per unitig reads its component's keys; summary: a lane per component, the counts and maxima through
//             per-workgroup slots and one reducing workgroup.
//
// Every loop is bounded by the unitigs, the components or constants.  Every index that comes from device data -- a record's
// position and target end, a parent, a root's rank, a component number -- is compared with its array's size before it
// addresses anything; a violation is counted in ctl[KMC_CC_BAD] and the host fails the call.
#pragma once
#include "kmc_clean.hip.h"

#define KMC_CC_THREADS KMC_C_THREADS   // (the block sums are c_block_add's)
#define KMC_CC_WAVES (KMC_CC_THREADS / 64)
#define KMC_CC_LEADERS 4
#define KMC_CC_ROUND_BATCH 4   // hook + shortcut rounds queued between two looks at their counters
// control words (u64): [0] the total of the scan = components (u32), [1] range violations, [2] components of one unitig,
// [3] the most keys, [4] the most unitigs in one component, [5] small components, [6] their keys; from [8] on the
// counters of a batch of rounds
#define KMC_CC_BAD 1
#define KMC_CC_SINGLE 2
#define KMC_CC_MAXKEYS 3
#define KMC_CC_MAXUNI 4
#define KMC_CC_SMALL 5
#define KMC_CC_SMALLKEYS 6
#define KMC_CC_ROUNDS_AT 8
#define KMC_CC_CTL_BYTES ((KMC_CC_ROUNDS_AT + KMC_CC_ROUND_BATCH) * sizeof(u64))
// a summary workgroup's slot: components of one unitig, small ones, their keys, the most keys, the most unitigs
#define KMC_CC_PART 8

__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_init_kernel(u32* __restrict__ parent, u64 nu) {
    const u64 u = (u64)blockIdx.x * KMC_CC_THREADS + threadIdx.x;
    if (u < nu) parent[u] = (u32)u;
}

// The root of x's tree as this lane sees it: at most nu steps, every parent checked (p <= x < nu) before it is followed.
__device__ __forceinline__ u32 cc_root(const u32* parent, u32 x, u64 nu, u32* bad) {
    for (u64 step = 0; step < nu; ++step) {
        const u32 p = parent[x];
        if (p == x) return x;
        if (p > x) { ++*bad; return x; }   // (x < nu, so p < nu from here on)
        x = p;
    }
    return x;
}

// the largest v of the workgroup, in thread 0 (ws: KMC_CC_WAVES words of LDS, free again on return; the sums go through
// c_block_add of kmc_clean.hip.h)
__device__ __forceinline__ u64 cc_block_max(u64 v, kmc_ull* ws) {
    const u32 tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(v, o); v = t > v ? t : v; }
    __syncthreads();
    if ((tid & 63) == 0) ws[tid >> 6] = v;
    __syncthreads();
    u64 s = 0;
    if (tid == 0) for (int q = 0; q < KMC_CC_WAVES; ++q) s = ws[q] > s ? ws[q] : s;
    return s;
}

// One hook pass: ends blockIdx.x * 256 + tid, + gridDim.x * 256, ...  *hooked += the atomics of this workgroup (one add
// per workgroup that issued any), ctl[KMC_CC_BAD] += range violations.
__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_hook_kernel(const u64* __restrict__ link_offsets, const u32* __restrict__ link_to, u64 nu, u64 n_links, u32* parent,
                        kmc_ull* __restrict__ hooked, kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull ws[KMC_CC_WAVES];
    const u64 n_ends = 2 * nu, stride = (u64)gridDim.x * KMC_CC_THREADS;
    u32 n_hook = 0, bad = 0;
    for (u64 e = (u64)blockIdx.x * KMC_CC_THREADS + threadIdx.x; e < n_ends; e += stride) {
        const u64 s0 = link_offsets[e], s1 = link_offsets[e + 1];
        if (s1 < s0 || s1 - s0 > 4 || s1 > n_links) { ++bad; continue; }
        if (s0 == s1) continue;
        const u32 u = (u32)(e >> 1);
        u32 ru = cc_root(parent, u, nu, &bad);
        for (u64 i = s0; i < s1; ++i) {   // (at most four)
            const u64 t = link_to[i];
            if (t >= n_ends) { ++bad; continue; }
            const u32 v = (u32)(t >> 1);
            if (v == u) continue;
            const u32 rv = cc_root(parent, v, nu, &bad);
            if (rv == ru) continue;
            const u32 lo = rv < ru ? rv : ru, hi = rv < ru ? ru : rv;
            atomicMin(&parent[hi], lo);
            ++n_hook;
            ru = lo;
        }
    }
    c_block_add((u64)n_hook, ws, hooked);
    c_block_add((u64)bad, ws, &ctl[KMC_CC_BAD]);
}

// One shortcut pass: parent[u] = the root of u's tree (u is the only writer of parent[u] in this launch).
__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_shortcut_kernel(u32* parent, u64 nu, kmc_ull* __restrict__ ctl) {
    const u64 u = (u64)blockIdx.x * KMC_CC_THREADS + threadIdx.x;
    u32 bad = 0;
    if (u < nu) {
        const u32 r = cc_root(parent, (u32)u, nu, &bad);
        if (r != parent[u]) parent[u] = r;
    }
    if (bad) atomicAdd(&ctl[KMC_CC_BAD], (kmc_ull)bad);
}

// is_root[u] for the scan; behind the last round every parent is a root
__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_flag_kernel(const u32* __restrict__ parent, u64 nu, u32* __restrict__ is_root, kmc_ull* __restrict__ ctl) {
    const u64 u = (u64)blockIdx.x * KMC_CC_THREADS + threadIdx.x;
    if (u >= nu) return;
    const u32 p = parent[u];
    const bool ok = (u64)p <= u && parent[p] == p;
    is_root[u] = p == (u32)u ? 1u : 0u;
    if (!ok) atomicAdd(&ctl[KMC_CC_BAD], 1ull);
}

// comp_of[u] = rank[parent[u]]; a root writes comp_stats[c][0]
__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_number_kernel(const u32* __restrict__ parent, const u32* __restrict__ rank, u64 nu, u64 n_comps, u32* __restrict__ comp_of,
                          kmc_ull* __restrict__ stats, kmc_ull* __restrict__ ctl) {
    const u64 u = (u64)blockIdx.x * KMC_CC_THREADS + threadIdx.x;
    if (u >= nu) return;
    const u32 p = parent[u];
    const u64 c = (u64)p < nu ? (u64)rank[p] : ~0ull;
    if (c >= n_comps) {
        comp_of[u] = 0;
        atomicAdd(&ctl[KMC_CC_BAD], 1ull);
        return;
    }
    comp_of[u] = (u32)c;
    if (p == (u32)u) stats[c * KMC_COMPONENT_STAT_WORDS + 0] = (kmc_ull)u;
}

// comp_stats[c][1..3] += (1, m_u, A_u) over the unitigs of c
__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_stats_kernel(const u64* __restrict__ offsets, const u64* __restrict__ abund, u64 km1, const u32* __restrict__ comp_of, u64 nu,
                         u64 n_comps, kmc_ull* __restrict__ stats, kmc_ull* __restrict__ ctl) {
    const u32 lane = threadIdx.x & 63;
    const u64 u = (u64)blockIdx.x * KMC_CC_THREADS + threadIdx.x;
    u64 c = ~0ull, m = 0, a = 0;
    bool mine = false;
    if (u < nu) {
        c = comp_of[u];
        if (c < n_comps) {
            mine = true;
            m = offsets[u + 1] - offsets[u] - km1;
            a = abund[u];
        } else {
            atomicAdd(&ctl[KMC_CC_BAD], 1ull);
        }
    }
    kmc_ull left = __ballot(mine);
    for (int it = 0; it < KMC_CC_LEADERS && left; ++it) {   // (wave-uniform: left comes from ballots alone)
        const int leader = __builtin_ctzll(left);
        const u64 cl = __shfl(c, leader);
        const bool same = mine && c == cl;
        const kmc_ull who = __ballot(same);
        const u64 sn = (u64)__popcll(who), sm = wave_sum_u64(same ? m : 0ull), sa = wave_sum_u64(same ? a : 0ull);
        if ((int)lane == leader) {
            kmc_ull* w = stats + cl * KMC_COMPONENT_STAT_WORDS;
            atomicAdd(w + 1, (kmc_ull)sn);
            atomicAdd(w + 2, (kmc_ull)sm);
            atomicAdd(w + 3, (kmc_ull)sa);
        }
        if (same) mine = false;
        left &= ~who;
    }
    if (mine) {
        kmc_ull* w = stats + c * KMC_COMPONENT_STAT_WORDS;
        atomicAdd(w + 1, 1ull);
        atomicAdd(w + 2, (kmc_ull)m);
        atomicAdd(w + 3, (kmc_ull)a);
    }
}

// verdict[u] = KMC_CLEAN_COMPONENT iff the keys of u's component are <= limit (limit 0: never; ~0: always)
__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_verdict_kernel(const u32* __restrict__ comp_of, const kmc_ull* __restrict__ stats, u64 nu, u64 n_comps, u64 limit,
                           uint8_t* __restrict__ verdict, kmc_ull* __restrict__ ctl) {
    const u64 u = (u64)blockIdx.x * KMC_CC_THREADS + threadIdx.x;
    if (u >= nu) return;
    const u64 c = comp_of[u];
    if (c >= n_comps) {
        verdict[u] = KMC_CLEAN_KEEP;
        atomicAdd(&ctl[KMC_CC_BAD], 1ull);
        return;
    }
    verdict[u] = limit && stats[c * KMC_COMPONENT_STAT_WORDS + 2] <= limit ? KMC_CLEAN_COMPONENT : KMC_CLEAN_KEEP;
}

// a lane per component (grid-stride), the totals of a workgroup into its slot part[blockIdx.x * KMC_CC_PART ..]
__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_summary_kernel(const kmc_ull* __restrict__ stats, u64 n_comps, u64 limit, kmc_ull* __restrict__ part) {
    __shared__ kmc_ull ws[KMC_CC_WAVES];
    u64 single = 0, small = 0, small_keys = 0, max_keys = 0, max_uni = 0;
    const u64 stride = (u64)gridDim.x * KMC_CC_THREADS;
    for (u64 c = (u64)blockIdx.x * KMC_CC_THREADS + threadIdx.x; c < n_comps; c += stride) {
        const u64 nu = stats[c * KMC_COMPONENT_STAT_WORDS + 1], keys = stats[c * KMC_COMPONENT_STAT_WORDS + 2];
        single += nu == 1 ? 1u : 0u;
        if (limit && keys <= limit) { ++small; small_keys += keys; }
        max_keys = keys > max_keys ? keys : max_keys;
        max_uni = nu > max_uni ? nu : max_uni;
    }
    kmc_ull* mine = part + (u64)blockIdx.x * KMC_CC_PART;
    c_block_add<true>(single, ws, mine + 0);
    c_block_add<true>(small, ws, mine + 1);
    c_block_add<true>(small_keys, ws, mine + 2);
    const u64 s3 = cc_block_max(max_keys, ws), s4 = cc_block_max(max_uni, ws);
    if (threadIdx.x == 0) { mine[3] = s3; mine[4] = s4; }
}

// one workgroup: the n_wg slots of part[] into the control words
__global__ __launch_bounds__(KMC_CC_THREADS)
void kmc_cc_reduce_kernel(const kmc_ull* __restrict__ part, u32 n_wg, kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull ws[KMC_CC_WAVES];
    u64 v[5] = {0, 0, 0, 0, 0};
    for (u32 i = threadIdx.x; i < n_wg; i += KMC_CC_THREADS) {
        const kmc_ull* p = part + (u64)i * KMC_CC_PART;
        v[0] += p[0]; v[1] += p[1]; v[2] += p[2];
        v[3] = p[3] > v[3] ? p[3] : v[3];
        v[4] = p[4] > v[4] ? p[4] : v[4];
    }
    c_block_add<true>(v[0], ws, &ctl[KMC_CC_SINGLE]);
    c_block_add<true>(v[1], ws, &ctl[KMC_CC_SMALL]);
    c_block_add<true>(v[2], ws, &ctl[KMC_CC_SMALLKEYS]);
    const u64 s3 = cc_block_max(v[3], ws), s4 = cc_block_max(v[4], ws);
    if (threadIdx.x == 0) { ctl[KMC_CC_MAXKEYS] = s3; ctl[KMC_CC_MAXUNI] = s4; }
}
