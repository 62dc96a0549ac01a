// kmc_spectrum.hip.h -- what users do first with a count table, on the sorted view kmc_finalize left in HBM
// (include/kmc.h: kmc_histogram, kmc_filter_device, kmc_export_filtered):
//
//   abundance histogram   hist[min(count, n_bins - 1)] += 1 for every key with min <= count <= max, plus the largest such count
//   count-range filter    the keys with min <= count <= max, in view order (stream compaction, reduce-then-scan)
//
// Both read the view's count array with 16-byte loads (two counts per lane).  The view's arrays are hipMalloc'd
// buffers (16-byte aligned); the histogram still takes a misaligned head element apart, the filter's host side
// checks the alignment.
//
// Histogram contention.  A spectrum puts most keys in its lowest bins: on the all-distinct input of the sort path EVERY
// count is 1, and one LDS atomic per key would send all 64 lanes of every wave to the same LDS word.  Bins 1..4 are
// therefore counted in registers (four u32 per lane, compare-and-add, no atomics at all) and folded into LDS once per
// wave at the end; only counts >= 5 take an LDS atomic (bins that fit the workgroup's LDS part) or a global one (the
// rest).  Each workgroup's LDS part is at most KMC_SPEC_LDS_BINS counters (64 KiB: two workgroups per CU fit the
// 160 KiB), and only its non-zero counters are added to the global histogram.
#pragma once
#include "kmc_device.hip.h"

#define KMC_SPEC_LDS_BINS 16384   // u32 counters of one workgroup's LDS histogram (64 KiB)
#define KMC_SPEC_LOW 4            // bins 1..KMC_SPEC_LOW counted in registers
#define KMC_SPEC_THREADS 256
#define KMC_FILT_THREADS 256
#define KMC_FILT_ROUNDS 4         // a filter tile = ROUNDS x 256 lanes x 2 entries (one 16-byte load of counts per lane and round)
#define KMC_FILT_TILE (KMC_FILT_ROUNDS * KMC_FILT_THREADS * 2)


struct SpecAcc {
    u32 low[KMC_SPEC_LOW];
    u64 mx;
};

// one count: in range -> its bin (registers / LDS / global), max
__device__ __forceinline__ void spec_add(u64 c, u64 lo_c, u64 hi_c, u32 n_bins, u32 lds_bins, u32* lds,
                                         kmc_ull* __restrict__ hist, SpecAcc& a) {
    if (c < lo_c || c > hi_c) return;
    a.mx = c > a.mx ? c : a.mx;
    const u32 b = c >= (u64)(n_bins - 1) ? n_bins - 1 : (u32)c;
    if (b >= 1 && b <= KMC_SPEC_LOW) {
#pragma unroll
        for (int i = 0; i < KMC_SPEC_LOW; ++i) a.low[i] += b == (u32)(i + 1) ? 1u : 0u;
    } else if (b < lds_bins) {
        atomicAdd(&lds[b], 1u);
    } else {
        atomicAdd(&hist[b], 1ull);
    }
}

// hist[n_bins] and *max_out zeroed by the host.  lds_bins = min(n_bins, KMC_SPEC_LDS_BINS) counters of dynamic LDS.
// head (0 or 1): cnt[0] is not 16-byte aligned and is taken apart; the pairs start at cnt + head.
__global__ __launch_bounds__(KMC_SPEC_THREADS)
void kmc_histogram_kernel(const u64* __restrict__ cnt, u64 n, u32 head, u64 lo_c, u64 hi_c, u32 n_bins, u32 lds_bins,
                          kmc_ull* __restrict__ hist, kmc_ull* __restrict__ max_out) {
    extern __shared__ __align__(16) u32 spec_lds[];
    __shared__ kmc_ull wmax[KMC_SPEC_THREADS / 64];
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (u32 i = tid; i < lds_bins; i += KMC_SPEC_THREADS) spec_lds[i] = 0;
    __syncthreads();
    SpecAcc a;
#pragma unroll
    for (int i = 0; i < KMC_SPEC_LOW; ++i) a.low[i] = 0;
    a.mx = 0;
    const u64 n_pairs = (n - head) >> 1;
    const kmc_ull2* p = reinterpret_cast<const kmc_ull2*>(cnt + head);
    const u64 stride = (u64)gridDim.x * KMC_SPEC_THREADS;
    u64 i = (u64)blockIdx.x * KMC_SPEC_THREADS + tid;
    // two independent 16-byte loads in flight per lane and trip
    for (; i + stride < n_pairs; i += 2 * stride) {
        const kmc_ull2 v0 = p[i], v1 = p[i + stride];
        spec_add(v0.x, lo_c, hi_c, n_bins, lds_bins, spec_lds, hist, a);
        spec_add(v0.y, lo_c, hi_c, n_bins, lds_bins, spec_lds, hist, a);
        spec_add(v1.x, lo_c, hi_c, n_bins, lds_bins, spec_lds, hist, a);
        spec_add(v1.y, lo_c, hi_c, n_bins, lds_bins, spec_lds, hist, a);
    }
    if (i < n_pairs) {
        const kmc_ull2 v0 = p[i];
        spec_add(v0.x, lo_c, hi_c, n_bins, lds_bins, spec_lds, hist, a);
        spec_add(v0.y, lo_c, hi_c, n_bins, lds_bins, spec_lds, hist, a);
    }
    if (blockIdx.x == 0 && tid == 0) {
        if (head) spec_add(cnt[0], lo_c, hi_c, n_bins, lds_bins, spec_lds, hist, a);
        if ((n - head) & 1) spec_add(cnt[n - 1], lo_c, hi_c, n_bins, lds_bins, spec_lds, hist, a);
    }
    // registers -> one LDS add per wave and low bin; wave max -> LDS -> one atomic per workgroup
#pragma unroll
    for (int b = 0; b < KMC_SPEC_LOW; ++b) {
        u32 s = a.low[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0 && s && (u32)(b + 1) < n_bins) {
            if ((u32)(b + 1) < lds_bins) atomicAdd(&spec_lds[b + 1], s);
            else atomicAdd(&hist[b + 1], (kmc_ull)s);
        }
    }
    u64 m = a.mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(m, o); m = t > m ? t : m; }
    if (lane == 0) wmax[wv] = m;
    __syncthreads();
    if (tid == 0) {
        kmc_ull w = wmax[0];
        for (int q = 1; q < KMC_SPEC_THREADS / 64; ++q) w = wmax[q] > w ? wmax[q] : w;
        if (w) atomicMax(max_out, w);
    }
    for (u32 b = tid; b < lds_bins; b += KMC_SPEC_THREADS) {
        const u32 v = spec_lds[b];
        if (v) atomicAdd(&hist[b], (kmc_ull)v);
    }
}

// ---- order-preserving filter: per-tile kept counts, exclusive scan of them (kmc_scan.hip.h), scatter ----
// Tile t covers entries [t * TILE, (t + 1) * TILE); in round r lane l of wave w holds the pair 2 * (r * 256 + w * 64 + l) + {0, 1}
// of the tile: entries in view order are round-major, then wave, then lane, then the pair's element -- which is the order of the
// scatter's positions (tile base + earlier rounds and waves + the lane's prefix in the wave's two ballots).
__device__ __forceinline__ bool filt_keep(u64 c, u64 lo_c, u64 hi_c) { return c >= lo_c && c <= hi_c; }

// n entries, n_tiles = ceil(n / TILE); cnt 16-byte aligned.  tile_cnt[t] = kept entries of tile t; *kept_total += their counts.
// A workgroup walks tiles blockIdx.x, + gridDim.x, ... and adds its sum of kept counts with ONE atomic at the end: one atomic
// per tile on the single kept_total word serialised a filter that keeps everything (5 ms instead of 1.07 for 831 M keys).
__global__ __launch_bounds__(KMC_FILT_THREADS)
void kmc_filter_count_kernel(const u64* __restrict__ cnt, u64 n, u64 n_tiles, u64 lo_c, u64 hi_c, u32* __restrict__ tile_cnt,
                             kmc_ull* __restrict__ kept_total) {
    __shared__ u32 wk[2][KMC_FILT_THREADS / 64];
    __shared__ kmc_ull ws[KMC_FILT_THREADS / 64];
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    u64 sum = 0;
    int par = 0;
    for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x, par ^= 1) {
        const u64 t0 = t * KMC_FILT_TILE;
        u32 kept = 0;
#pragma unroll
        for (int r = 0; r < KMC_FILT_ROUNDS; ++r) {
            const u64 e = t0 + 2 * ((u64)r * KMC_FILT_THREADS + tid);
            kmc_ull2 v = {0ull, 0ull};
            bool k0 = false, k1 = false;
            if (e + 1 < n) { v = *reinterpret_cast<const kmc_ull2*>(cnt + e); k0 = filt_keep(v.x, lo_c, hi_c); k1 = filt_keep(v.y, lo_c, hi_c); }
            else if (e < n) { v.x = cnt[e]; k0 = filt_keep(v.x, lo_c, hi_c); }
            kept += (u32)__popcll(__ballot(k0)) + (u32)__popcll(__ballot(k1));
            sum += (k0 ? v.x : 0ull) + (k1 ? v.y : 0ull);
        }
        // (two LDS slots alternate between tiles: a wave may write the next tile's count while thread 0 still reads these)
        if (lane == 0) wk[par][wv] = kept;
        __syncthreads();
        if (tid == 0) {
            u32 k = 0;
            for (int q = 0; q < KMC_FILT_THREADS / 64; ++q) k += wk[par][q];
            tile_cnt[t] = k;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) ws[wv] = sum;
    __syncthreads();
    if (tid == 0) {
        kmc_ull s = 0;
        for (int q = 0; q < KMC_FILT_THREADS / 64; ++q) s += ws[q];
        if (s) atomicAdd(kept_total, s);
    }
}

// tile_base[t] = exclusive prefix of tile_cnt.  Keys: hi (KW == 2 only) and lo; all view arrays 16-byte aligned.
template <int KW>
__global__ __launch_bounds__(KMC_FILT_THREADS)
void kmc_filter_scatter_kernel(const u64* __restrict__ khi, const u64* __restrict__ klo, const u64* __restrict__ cnt, u64 n,
                               u64 lo_c, u64 hi_c, const u32* __restrict__ tile_base,
                               u64* __restrict__ ohi, u64* __restrict__ olo, u64* __restrict__ ocnt) {
    __shared__ u32 wk[KMC_FILT_ROUNDS * (KMC_FILT_THREADS / 64)];
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 t0 = (u64)blockIdx.x * KMC_FILT_TILE;
    kmc_ull2 vc[KMC_FILT_ROUNDS];
    kmc_ull m0[KMC_FILT_ROUNDS], m1[KMC_FILT_ROUNDS];
#pragma unroll
    for (int r = 0; r < KMC_FILT_ROUNDS; ++r) {
        const u64 e = t0 + 2 * ((u64)r * KMC_FILT_THREADS + tid);
        kmc_ull2 v = {0ull, 0ull};
        bool k0 = false, k1 = false;
        if (e + 1 < n) { v = *reinterpret_cast<const kmc_ull2*>(cnt + e); k0 = filt_keep(v.x, lo_c, hi_c); k1 = filt_keep(v.y, lo_c, hi_c); }
        else if (e < n) { v.x = cnt[e]; k0 = filt_keep(v.x, lo_c, hi_c); }
        vc[r] = v;
        m0[r] = __ballot(k0);
        m1[r] = __ballot(k1);
        if (lane == 0) wk[r * (KMC_FILT_THREADS / 64) + wv] = (u32)__popcll(m0[r]) + (u32)__popcll(m1[r]);
    }
    __syncthreads();
    // (round, wave) slots before this wave's slot of round 0
    u32 pos = tile_base[blockIdx.x];
    for (u32 q = 0; q < wv; ++q) pos += wk[q];
#pragma unroll
    for (int r = 0; r < KMC_FILT_ROUNDS; ++r) {
        const kmc_ull mr0 = m0[r], mr1 = m1[r];
        if (mr0 | mr1) {
            const bool k0 = (mr0 >> lane) & 1ull, k1 = (mr1 >> lane) & 1ull;
            // v_mbcnt: kept entries of the lanes below this one, both elements of their pairs
            const u32 below = __builtin_amdgcn_mbcnt_hi((u32)(mr0 >> 32), __builtin_amdgcn_mbcnt_lo((u32)mr0, 0u)) +
                              __builtin_amdgcn_mbcnt_hi((u32)(mr1 >> 32), __builtin_amdgcn_mbcnt_lo((u32)mr1, 0u));
            if (k0 | k1) {
                const u64 e = t0 + 2 * ((u64)r * KMC_FILT_THREADS + tid);
                u64 o = (u64)pos + below;
                kmc_ull2 vl, vh = {0ull, 0ull};
                if (e + 1 < n) {
                    vl = *reinterpret_cast<const kmc_ull2*>(klo + e);
                    if (KW == 2) vh = *reinterpret_cast<const kmc_ull2*>(khi + e);
                } else {
                    vl.x = klo[e]; vl.y = 0;
                    if (KW == 2) vh.x = khi[e];
                }
                if (k0) { olo[o] = vl.x; ocnt[o] = vc[r].x; if (KW == 2) ohi[o] = vh.x; ++o; }
                if (k1) { olo[o] = vl.y; ocnt[o] = vc[r].y; if (KW == 2) ohi[o] = vh.y; }
            }
        }
        // the rest of this round (later waves) and the earlier waves of the next round
        if (r + 1 < KMC_FILT_ROUNDS)
            for (u32 q = wv; q < wv + KMC_FILT_THREADS / 64; ++q) pos += wk[r * (KMC_FILT_THREADS / 64) + q];
    }
}
