// kmc_setops.hip.h -- two count tables compared on the device (include/kmc.h: kmc_compare, kmc_setop_device,
// kmc_export_setop).  A and B are sorted views: ascending, unique keys.  For a key x, ca = its count in A if it lies in
// [min_a, max_a], else 0; cb likewise.  Every key of either view is seen once with its (ca, cb):
//
//   summary (8 words)   n_a, n_b, n_both, sum ca, sum cb, sum ca / sum cb over shared keys, sum min(ca, cb)
//   set operation       the keys an op selects, with the count a count mode gives them, in key order (r != 0 only)
//
// Merge-path tiling.  The MERGED sequence (A first on equal keys) is cut into tiles of KMC_SO_TILE elements; one thread per
// tile boundary finds by binary search over the two views where that diagonal crosses them (kmc_setop_partition_kernel).
// Cost is therefore per merged element, whatever the skew: one key against two million, disjoint ranges and strict
// interleaving all make the same tiles.  Keys are unique within a view, so a boundary can separate at most the A copy and
// the B copy of one equal key: then the B copy is moved into the earlier tile (a tile holds at most TILE + 1 elements).
// Inside a tile both segments are streamed into LDS with 16-byte loads, every thread repeats the diagonal search for its
// KMC_SO_ITEMS elements in LDS (same tie rule, same fix) and merges them serially.
//
//   kmc_setop_join_kernel<KW, 0>  compare: the summary only; wave reduction, one set of atomics per workgroup
//   kmc_setop_join_kernel<KW, 1>  count:   the same plus emitted keys per tile (scanned by kmc_scan.hip.h) and sum of r
//   kmc_setop_join_kernel<KW, 2>  scatter: emitted entries compacted in LDS, copied out coalesced at the tile's base
#pragma once
#include "kmc_device.hip.h"

#define KMC_SO_THREADS 256
#define KMC_SO_ITEMS 6
#define KMC_SO_TILE (KMC_SO_THREADS * KMC_SO_ITEMS)   // merged elements per tile (the tests' boundary cases assume 1536)
#define KMC_SO_CAP (KMC_SO_TILE + 2)                  // LDS entries: TILE + 1 at most, kept even
#define KMC_SO_WORDS 9                                // device accumulators: the 8 summary words, then sum of r (total_out)

struct SoView : KView { u64 min_c, max_c; };   // count range (max_c: ~0 for "no upper bound")

template <int KW>
__device__ __forceinline__ bool so_less(u64 h1, u64 l1, u64 h2, u64 l2) {
    return KW == 2 ? key_less(h1, l1, h2, l2) : l1 < l2;   // (one-word keys: the high words are not looked at)
}
template <int KW>
__device__ __forceinline__ bool so_equal(u64 h1, u64 l1, u64 h2, u64 l2) {
    return KW == 2 ? key_equal(h1, l1, h2, l2) : l1 == l2;
}

// Where diagonal d of the merged sequence crosses A (na keys) and B (nb keys): ia + ib == d, A first on equal keys.
// If that separates the two copies of one key (A[ia - 1] == B[ib]), the B copy goes with the A copy: ib + 1.
template <int KW>
__device__ __forceinline__ void so_split(const u64* ahi, const u64* alo, u32 na, const u64* bhi, const u64* blo, u32 nb, u32 d,
                                         u32& ia, u32& ib) {
    u32 lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1, j = d - 1 - mid;
        const bool b_first = so_less<KW>(KW == 2 ? bhi[j] : 0ull, blo[j], KW == 2 ? ahi[mid] : 0ull, alo[mid]);
        if (b_first) hi = mid; else lo = mid + 1;
    }
    u32 b = d - lo;
    if (lo > 0 && b < nb && so_equal<KW>(KW == 2 ? ahi[lo - 1] : 0ull, alo[lo - 1], KW == 2 ? bhi[b] : 0ull, blo[b])) ++b;
    ia = lo;
    ib = b;
}

// pa[t], pb[t], t = 0..n_tiles: first A / B entry of tile t (entry n_tiles: the views' ends).  na + nb < 2^32.
template <int KW>
__global__ __launch_bounds__(256)
void kmc_setop_partition_kernel(SoView A, SoView B, u32 n_tiles, u32* __restrict__ pa, u32* __restrict__ pb) {
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (t > n_tiles) return;
    const u64 nm = A.n + B.n, dd = (u64)t * KMC_SO_TILE;
    u32 ia, ib;
    so_split<KW>(A.hi, A.lo, (u32)A.n, B.hi, B.lo, (u32)B.n, (u32)(dd < nm ? dd : nm), ia, ib);
    pa[t] = ia;
    pb[t] = ib;
}

// src[s, s + len) -> dst[0, len) (LDS) with 16-byte loads of the aligned pairs that cover it; n = length of src.
__device__ __forceinline__ void so_stage(const u64* __restrict__ src, u64 n, u32 s, u32 len, u64* dst, u32 tid) {
    if (!len) return;
    const u32 e0 = s & ~1u, n_pairs = (s + len - e0 + 1) >> 1;
    for (u32 p = tid; p < n_pairs; p += KMC_SO_THREADS) {
        const u32 e = e0 + 2 * p;
        kmc_ull2 v = {0ull, 0ull};
        if ((u64)e + 1 < n) v = *reinterpret_cast<const kmc_ull2*>(src + e);
        else v.x = src[e];
        if (e >= s) dst[e - s] = v.x;
        if (e + 1 < s + len) dst[e + 1 - s] = v.y;
    }
}

struct SoAcc { u64 w[KMC_SO_WORDS]; };

__device__ __forceinline__ u64 so_result(int mode, u64 ca, u64 cb) {
    switch (mode) {
        case 0: return ca;
        case 1: return cb;
        case 2: return ca < cb ? ca : cb;
        case 3: return ca > cb ? ca : cb;
        case 4: return ca + cb;
        default: return ca > cb ? ca - cb : 0ull;
    }
}

// One thread's share of a tile: A entries [a, ea) and B entries [b, eb) of the LDS segments, merged.  Adds to the summary
// (ACC), counts the emitted keys, and (EMIT) writes them to the LDS output arrays from slot o on.  Returns the emitted keys.
template <int KW, bool ACC, bool EMIT>
__device__ __forceinline__ u32 so_merge(const u64* khi, const u64* klo, const u64* kc, u32 nat, u32 a, u32 ea, u32 b, u32 eb,
                                        u64 min_a, u64 max_a, u64 min_b, u64 max_b, int op, int mode, SoAcc& acc,
                                        u64* ohi, u64* olo, u64* oc, u32 o) {
    u32 emitted = 0;
    while (a < ea || b < eb) {
        const bool ha = a < ea, hb = b < eb;
        const u32 ja = ha ? a : 0u, jb = hb ? nat + b : 0u;   // (slot 0 is always readable)
        const u64 ah = KW == 2 ? khi[ja] : 0ull, al = klo[ja], bh = KW == 2 ? khi[jb] : 0ull, bl = klo[jb];
        const bool take_a = ha && (!hb || !so_less<KW>(bh, bl, ah, al));
        const bool take_b = hb && (!ha || !so_less<KW>(ah, al, bh, bl));
        u64 ca = take_a ? kc[ja] : 0ull, cb = take_b ? kc[jb] : 0ull;
        ca = (ca >= min_a && ca <= max_a) ? ca : 0ull;
        cb = (cb >= min_b && cb <= max_b) ? cb : 0ull;
        a += take_a ? 1u : 0u;
        b += take_b ? 1u : 0u;
        const bool in_a = ca != 0, in_b = cb != 0, both = in_a && in_b;
        const bool sel = op == 0 ? both : op == 1 ? (in_a || in_b) : (in_a && !in_b);
        const u64 r = sel ? so_result(mode, ca, cb) : 0ull;
        if (ACC) {
            acc.w[0] += in_a ? 1ull : 0ull;
            acc.w[1] += in_b ? 1ull : 0ull;
            acc.w[2] += both ? 1ull : 0ull;
            acc.w[3] += ca;
            acc.w[4] += cb;
            acc.w[5] += both ? ca : 0ull;
            acc.w[6] += both ? cb : 0ull;
            acc.w[7] += both ? (ca < cb ? ca : cb) : 0ull;
            acc.w[8] += r;
        }
        if (r) {
            if (EMIT) {
                if (KW == 2) ohi[o + emitted] = take_a ? ah : bh;
                olo[o + emitted] = take_a ? al : bl;
                oc[o + emitted] = r;
            }
            ++emitted;
        }
    }
    return emitted;
}

// PASS 0: compare (summary), 1: count (summary, tile_cnt), 2: scatter (tile_base = exclusive scan of tile_cnt -> out arrays).
// acc_out[KMC_SO_WORDS] zeroed by the host (passes 0 and 1).  Workgroups walk tiles blockIdx.x, + gridDim.x, ...
template <int KW, int PASS>
__global__ __launch_bounds__(KMC_SO_THREADS)
void kmc_setop_join_kernel(SoView A, SoView B, int op, int mode, u32 n_tiles, const u32* __restrict__ pa, const u32* __restrict__ pb,
                           u32* __restrict__ tile_cnt, const u32* __restrict__ tile_base, kmc_ull* __restrict__ acc_out,
                           u64* __restrict__ out_hi, u64* __restrict__ out_lo, u64* __restrict__ out_cnt) {
    __shared__ __align__(16) u64 s_lo[KMC_SO_CAP];
    __shared__ __align__(16) u64 s_hi[KW == 2 ? KMC_SO_CAP : 2];
    __shared__ __align__(16) u64 s_c[KMC_SO_CAP];
    __shared__ __align__(16) u64 o_lo[PASS == 2 ? KMC_SO_CAP : 2];
    __shared__ __align__(16) u64 o_hi[PASS == 2 && KW == 2 ? KMC_SO_CAP : 2];
    __shared__ __align__(16) u64 o_c[PASS == 2 ? KMC_SO_CAP : 2];
    __shared__ u32 s_a[KMC_SO_THREADS + 1], s_b[KMC_SO_THREADS + 1];
    __shared__ u32 s_wv[KMC_SO_THREADS / 64];
    __shared__ kmc_ull s_acc[KMC_SO_THREADS / 64][KMC_SO_WORDS];
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    SoAcc acc;
#pragma unroll
    for (int i = 0; i < KMC_SO_WORDS; ++i) acc.w[i] = 0;

    for (u32 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const u32 a0 = pa[t], b0 = pb[t], nat = pa[t + 1] - a0, nbt = pb[t + 1] - b0, nt = nat + nbt;   // nt <= TILE + 1
        if (KW == 2) { so_stage(A.hi, A.n, a0, nat, s_hi, tid); so_stage(B.hi, B.n, b0, nbt, s_hi + nat, tid); }
        so_stage(A.lo, A.n, a0, nat, s_lo, tid);
        so_stage(B.lo, B.n, b0, nbt, s_lo + nat, tid);
        so_stage(A.cnt, A.n, a0, nat, s_c, tid);
        so_stage(B.cnt, B.n, b0, nbt, s_c + nat, tid);
        __syncthreads();
        {
            const u32 d = tid * KMC_SO_ITEMS < nt ? tid * KMC_SO_ITEMS : nt;
            u32 ia, ib;
            so_split<KW>(s_hi, s_lo, nat, s_hi + nat, s_lo + nat, nbt, d, ia, ib);
            s_a[tid] = ia;
            s_b[tid] = ib;
            if (tid == 0) { s_a[KMC_SO_THREADS] = nat; s_b[KMC_SO_THREADS] = nbt; }
        }
        __syncthreads();
        const u32 a = s_a[tid], ea = s_a[tid + 1], b = s_b[tid], eb = s_b[tid + 1];
        const u32 mine = so_merge<KW, PASS != 2, false>(s_hi, s_lo, s_c, nat, a, ea, b, eb, A.min_c, A.max_c, B.min_c, B.max_c, op, mode, acc,
                                                        nullptr, nullptr, nullptr, 0u);
        if (PASS != 0) {
            // emitted keys of the threads before this one (wave scan, then the earlier waves), and of the tile
            u32 inc = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const u32 v = __shfl_up(inc, o); if (lane >= (u32)o) inc += v; }
            if (lane == 63) s_wv[wv] = inc;
            __syncthreads();
            u32 before = inc - mine, total = 0;
#pragma unroll
            for (u32 q = 0; q < KMC_SO_THREADS / 64; ++q) { const u32 v = s_wv[q]; before += q < wv ? v : 0u; total += v; }
            if (PASS == 1) {
                if (tid == 0) tile_cnt[t] = total;
            } else {
                so_merge<KW, false, true>(s_hi, s_lo, s_c, nat, a, ea, b, eb, A.min_c, A.max_c, B.min_c, B.max_c, op, mode, acc, o_hi, o_lo, o_c, before);
                __syncthreads();
                const u64 base = tile_base[t];
                for (u32 i = tid; i < total; i += KMC_SO_THREADS) {
                    if (KW == 2) out_hi[base + i] = o_hi[i];
                    out_lo[base + i] = o_lo[i];
                    out_cnt[base + i] = o_c[i];
                }
            }
        }
        __syncthreads();   // (the next tile overwrites the LDS segments, s_a / s_b, s_wv and the output arrays)
    }

    if (PASS != 2) {
#pragma unroll
        for (int i = 0; i < KMC_SO_WORDS; ++i) {
            u64 s = acc.w[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) s_acc[wv][i] = s;
        }
        __syncthreads();
        if (tid < KMC_SO_WORDS) {
            kmc_ull s = 0;
            for (int q = 0; q < KMC_SO_THREADS / 64; ++q) s += s_acc[q][tid];
            if (s) atomicAdd(&acc_out[tid], s);
        }
    }
}
