// kmc_clean.hip.h -- cleaning the compacted graph (include/kmc.h: kmc_unitig_clean, kmc_unitig_clean_device,
// kmc_unitig_clean_into and their kmc_unitig_simplify* forms): a verdict per unitig -- keep, tip, island, and for a simplify
// call bubble -- and the table of the keys of the kept unitigs.
//
// What a links call leaves on the device is all this needs: the unitig arrays (offsets, abund, flags), the link records
// (link_offsets per end, link_to), and per view row adj, the final ranking (ptr) and uid_of (kmc_links.hip.h).
//   verdict   a lane per unitig.  It decides island and tip candidate from its own sizes and record counts, follows the one
//             record of its attached end, walks the at most four records of the end it reaches and decides every sibling's
//             candidacy the same way.  Mean abundances are compared as 128-bit products.  With BUBBLES a unitig with one
//             record at each end also follows both, walks the at most four records of the end its START end reaches and asks
//             of every sibling whether it is a candidate between the same two ends that beats it.  Without BUBBLES none of
//             that is compiled: a kmc_unitig_clean* call runs the kernels it always ran.
//   mark      a lane per view row, tiles of KMC_C_TILE rows: a solid row finds its unitig (the first-key row from its ranking
//             entry, uid_of) and that unitig's verdict; the class goes into one byte per row, the kept rows are counted per
//             tile, and the key totals per class and the sum of the kept counts are added up per workgroup (with BUBBLES
//             also the keys of class 3 and the sum of their counts).
//   scatter   behind the exclusive scan of the tile counts: the same tiles, the class bytes alone decide; a kept row is
//             written at tile base + earlier (round, wave) slots + the lane's prefix in its wave's ballot, which is view order.
//
// No kernel waits for another workgroup and every loop is bounded by the view, the unitigs or constants.  Every index that
// comes from device data -- a record's position and target end, a sibling end, a first-key row, a unitig id, a scatter
// position -- is compared with its array's size before it addresses anything; a violation is counted in ctl[KMC_C_BAD] and
// the host fails the call.
#pragma once
#include "kmc_unitig.hip.h"

#define KMC_C_THREADS 256
#define KMC_C_WAVES (KMC_C_THREADS / 64)
#define KMC_C_ROUNDS 4
#define KMC_C_TILE (KMC_C_ROUNDS * KMC_C_THREADS)
#define KMC_C_WORDS 8      // KMC_CLEAN_WORDS
// control words: [0] the total of the scan (u32), [1 + i] summary word i < 8, [9] range violations, [10 + i] summary word
// 8 + i of a simplify call (bubbles, their keys, bubble candidates, the counts of their keys)
#define KMC_C_SUM 1
#define KMC_C_BAD 9
#define KMC_C_SUM2 10
#define KMC_C_CTL_WORDS 14
// a row's class byte: not solid, or solid with its unitig's verdict
#define KMC_C_ROW_NONE 0xFFu

struct CleanGraph {
    const u64* offsets;        // n_unitigs + 1
    const u64* abund;          // n_unitigs
    const uint8_t* flags;      // n_unitigs
    const u64* link_offsets;   // 2 * n_unitigs + 1
    const u32* link_to;        // n_links
    u64 n_unitigs, n_links;
    u64 km1;                   // k - 1
    u64 max_tip, max_island, max_bubble;
};

// What the rule asks of a unitig: its keys and abundance, the records at its two ends, and from them whether it is a tip
// candidate and through which end it is attached.  w < n_unitigs.
struct CUnit { u64 m, abund, r0, r1, o0, o1; bool circ, cand; u32 attached; };
__device__ __forceinline__ CUnit c_unit(const CleanGraph& g, u64 w) {
    CUnit x;
    x.m = g.offsets[w + 1] - g.offsets[w] - g.km1;
    x.abund = g.abund[w];
    x.circ = (g.flags[w] & 1u) != 0;
    const u64 o0 = g.link_offsets[2 * w], o1 = g.link_offsets[2 * w + 1], o2 = g.link_offsets[2 * w + 2];
    x.r0 = o1 - o0;
    x.r1 = o2 - o1;
    x.o0 = o0;
    x.o1 = o1;
    x.cand = !x.circ && x.m <= g.max_tip && ((x.r0 == 0 && x.r1 == 1) || (x.r0 == 1 && x.r1 == 0));
    x.attached = (u32)(2 * w) + (x.r1 == 1 ? 1u : 0u);
    return x;
}

// w beats u among candidates: higher mean abundance (A_w / m_w > A_u / m_u as 128-bit products), then more keys, then the
// smaller id
__device__ __forceinline__ bool c_beats(const CUnit& w, u64 wid, const CUnit& u, u64 uid) {
    const unsigned __int128 l = (unsigned __int128)w.abund * u.m, r = (unsigned __int128)u.abund * w.m;
    if (l != r) return l > r;
    if (w.m != u.m) return w.m > u.m;
    return wid < uid;
}

// The one record at each end of a unit with r0 == r1 == 1, if it makes the unit a bubble candidate: both records inside
// their arrays (else *bad), different from one another and neither an end of the unit itself.  x.m <= max_bubble and
// !x.circ are the caller's to ask first.
__device__ __forceinline__ bool c_bubble_ends(const CleanGraph& g, const CUnit& x, u64 id, u64 n_ends, u64* p, u64* q, u32* bad) {
    if (x.o0 >= g.n_links || x.o1 >= g.n_links) { ++*bad; return false; }
    *p = g.link_to[x.o0];
    *q = g.link_to[x.o1];
    if (*p >= n_ends || *q >= n_ends) { ++*bad; return false; }
    return *p != *q && (*p >> 1) != id && (*q >> 1) != id;
}

// verdict[u] for every unitig; ctl[KMC_C_SUM + 1] tips, [+ 2] islands, [+ 6] tip candidates, with BUBBLES
// ctl[KMC_C_SUM2 + 0] bubbles and [+ 2] bubble candidates; one atomic per wave and word
template <bool BUBBLES>
__global__ __launch_bounds__(KMC_C_THREADS)
void kmc_clean_verdict_kernel(CleanGraph g, uint8_t* __restrict__ verdict, kmc_ull* __restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    const u64 u = (u64)blockIdx.x * KMC_C_THREADS + threadIdx.x;
    const u64 n_ends = 2 * g.n_unitigs;
    u32 tip = 0, island = 0, cand = 0, bad = 0, bubble = 0, bcand = 0;
    if (u < g.n_unitigs) {
        const CUnit me = c_unit(g, u);
        uint8_t v = KMC_CLEAN_KEEP;
        if (!me.circ && me.r0 == 0 && me.r1 == 0 && me.m <= g.max_island) {
            v = KMC_CLEAN_ISLAND;
            island = 1;
        } else if (me.cand) {
            cand = 1;
            const u32 a = me.attached;
            const u64 at = g.link_offsets[a];
            const u64 t = at < g.n_links ? (u64)g.link_to[at] : ~0ull;
            if (t >= n_ends) {
                ++bad;
            } else {
                const u64 s0 = g.link_offsets[t], s1 = g.link_offsets[t + 1];
                if (s1 < s0 || s1 - s0 > 4 || s1 > g.n_links) {
                    ++bad;
                } else {
                    bool dominated = false;
                    for (u64 i = s0; i < s1; ++i) {   // (at most four)
                        const u64 s = g.link_to[i];
                        if (s >= n_ends) { ++bad; continue; }
                        const u64 w = s >> 1;
                        if (s == (u64)a || w == u) continue;
                        const CUnit sib = c_unit(g, w);
                        dominated = dominated || !sib.cand || c_beats(sib, w, me, u);
                    }
                    if (dominated) { v = KMC_CLEAN_TIP; tip = 1; }
                }
            }
        } else if (BUBBLES && !me.circ && me.r0 == 1 && me.r1 == 1 && me.m <= g.max_bubble) {
            u64 p = 0, q = 0;
            if (c_bubble_ends(g, me, u, n_ends, &p, &q, &bad)) {
                bcand = 1;
                const u64 s0 = g.link_offsets[p], s1 = g.link_offsets[p + 1];
                if (s1 < s0 || s1 - s0 > 4 || s1 > g.n_links) {
                    ++bad;
                } else {
                    bool beaten = false;
                    for (u64 i = s0; i < s1; ++i) {   // (at most four)
                        const u64 s = g.link_to[i];
                        if (s >= n_ends) { ++bad; continue; }
                        const u64 w = s >> 1;
                        if (w == u) continue;
                        const CUnit sib = c_unit(g, w);
                        if (sib.circ || sib.r0 != 1 || sib.r1 != 1 || sib.m > g.max_bubble) continue;
                        u64 wp = 0, wq = 0;
                        if (!c_bubble_ends(g, sib, w, n_ends, &wp, &wq, &bad)) continue;
                        const bool parallel = (wp == p && wq == q) || (wp == q && wq == p);
                        beaten = beaten || (parallel && c_beats(sib, w, me, u));
                    }
                    if (beaten) { v = KMC_CLEAN_BUBBLE; bubble = 1; }
                }
            }
        }
        verdict[u] = v;
    }
    const u64 st = wave_sum_u64((u64)tip), si = wave_sum_u64((u64)island), sc = wave_sum_u64((u64)cand), sb = wave_sum_u64((u64)bad);
    if (lane == 0) {
        if (st) atomicAdd(&ctl[KMC_C_SUM + 1], (kmc_ull)st);
        if (si) atomicAdd(&ctl[KMC_C_SUM + 2], (kmc_ull)si);
        if (sc) atomicAdd(&ctl[KMC_C_SUM + 6], (kmc_ull)sc);
        if (sb) atomicAdd(&ctl[KMC_C_BAD], (kmc_ull)sb);
    }
    if (BUBBLES) {
        const u64 sp = wave_sum_u64((u64)bubble), sq = wave_sum_u64((u64)bcand);
        if (lane == 0) {
            if (sp) atomicAdd(&ctl[KMC_C_SUM2 + 0], (kmc_ull)sp);
            if (sq) atomicAdd(&ctl[KMC_C_SUM2 + 2], (kmc_ull)sq);
        }
    }
}

// sums of the four waves of a workgroup, added to *dst by thread 0 -- or, with STORE, written there (ws: KMC_C_WAVES words
// of LDS, free again on return)
template <bool STORE = false>
__device__ __forceinline__ void c_block_add(u64 v, kmc_ull* ws, kmc_ull* dst) {
    const u32 tid = threadIdx.x;
    v = wave_sum_u64(v);
    __syncthreads();
    if ((tid & 63) == 0) ws[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        kmc_ull s = 0;
        for (int q = 0; q < KMC_C_WAVES; ++q) s += ws[q];
        if (STORE) *dst = s;
        else if (s) atomicAdd(dst, s);
    }
}

// The totals of a mark<true> workgroup: KMC_C_PART words in its own slot of part[], which kmc_clean_reduce_kernel adds up.
// (Where bubbles are popped nearly every workgroup has every total non-zero, and some thousand atomics on the one cache
// line of the control words then take as long as the kernel's reads: DESIGN 4.14.)
#define KMC_C_PART 8

// the row of the first key of the unitig a solid row belongs to, from the two entries of the ranking alone (u_place's rule)
__device__ __forceinline__ u32 c_first_row(uint2 e, bool canon) {
    const u32 er = e.x >> 1, el = e.y >> 1;
    return canon && er < el ? er : el;
}

// The mark and count pass.  row_class[r] = the verdict of row r's unitig, KMC_C_ROW_NONE for a row that is not solid;
// tile_cnt[t] = kept rows of tile t; ctl[KMC_C_SUM + 3 / 4 / 5] += keys kept / of tips / of islands, [+ 7] += the counts of
// the kept keys.  A workgroup walks tiles blockIdx.x, + gridDim.x, ... and adds its totals once at the end.
// A row's class is three loads behind one another -- its ranking entry, uid_of of the first-key row, that unitig's verdict.
// The four rows a lane has in a tile go through each step together, without a branch between the loads, so that the loads
// of a step are in flight at once; the ranking and count of a row that is not solid are read and ignored (both arrays
// cover every view row).  With BUBBLES the keys of bubbles and the counts of those keys are summed too, and the totals
// go to the workgroup's slot part[blockIdx.x * KMC_C_PART ..] instead of to ctl (the order: kmc_clean_reduce_kernel).
template <bool BUBBLES>
__global__ __launch_bounds__(KMC_C_THREADS)
void kmc_clean_mark_kernel(const u64* __restrict__ cnt, u64 n, u64 n_tiles, const uint16_t* __restrict__ adj, const u32* __restrict__ ptr,
                           const u32* __restrict__ uid_of, int canon, const uint8_t* __restrict__ verdict,
                           u64 n_unitigs, uint8_t* __restrict__ row_class, u32* __restrict__ tile_cnt, kmc_ull* __restrict__ ctl,
                           kmc_ull* __restrict__ part) {
    __shared__ u32 wk[2][KMC_C_WAVES];
    __shared__ kmc_ull ws[KMC_C_WAVES];
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    u64 sum = 0, n_keep = 0, n_tip = 0, n_isl = 0, n_bad = 0, n_bub = 0, sum_bub = 0;
    int par = 0;
    for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x, par ^= 1) {
        const u64 e0 = t * KMC_C_TILE + tid;
        bool solid[KMC_C_ROUNDS];
        uint2 pe[KMC_C_ROUNDS];
        u64 cv[KMC_C_ROUNDS];
        u32 id[KMC_C_ROUNDS];
        uint8_t cls[KMC_C_ROUNDS];
#pragma unroll
        for (int r = 0; r < KMC_C_ROUNDS; ++r) {
            const u64 e = e0 + (u64)r * KMC_C_THREADS;
            const bool in = e < n;
            solid[r] = in && (((u32)adj[in ? e : 0] >> 10) & 1u);
            pe[r] = reinterpret_cast<const uint2*>(ptr)[in ? e : 0];
            cv[r] = cnt[in ? e : 0];
        }
#pragma unroll
        for (int r = 0; r < KMC_C_ROUNDS; ++r) {
            const u32 first = c_first_row(pe[r], canon != 0);
            const bool ok = solid[r] && first < n;
            id[r] = uid_of[ok ? first : 0];
            if (!ok) id[r] = KMC_U_NONE;
        }
#pragma unroll
        for (int r = 0; r < KMC_C_ROUNDS; ++r) {
            const bool ok = (u64)id[r] < n_unitigs;
            const uint8_t v = verdict[ok ? id[r] : 0];
            cls[r] = !solid[r] ? (uint8_t)KMC_C_ROW_NONE : ok ? v : (uint8_t)KMC_C_ROW_NONE;
            n_bad += solid[r] && !ok ? 1u : 0u;
        }
        u32 kept = 0;
#pragma unroll
        for (int r = 0; r < KMC_C_ROUNDS; ++r) {
            const u64 e = e0 + (u64)r * KMC_C_THREADS;
            if (e < n) row_class[e] = cls[r];
            const bool keep = cls[r] == KMC_CLEAN_KEEP;
            sum += keep ? cv[r] : 0ull;
            n_keep += keep ? 1u : 0u;
            n_tip += cls[r] == KMC_CLEAN_TIP ? 1u : 0u;
            n_isl += cls[r] == KMC_CLEAN_ISLAND ? 1u : 0u;
            if (BUBBLES) {
                const bool bub = cls[r] == KMC_CLEAN_BUBBLE;
                n_bub += bub ? 1u : 0u;
                sum_bub += bub ? cv[r] : 0ull;
            }
            kept += (u32)__popcll(__ballot(keep));
        }
        // (two LDS slots alternate between tiles: a wave may write the next tile's count while thread 0 still reads these)
        if (lane == 0) wk[par][wv] = kept;
        __syncthreads();
        if (tid == 0) {
            u32 k = 0;
            for (int q = 0; q < KMC_C_WAVES; ++q) k += wk[par][q];
            tile_cnt[t] = k;
        }
    }
    if (BUBBLES) {
        kmc_ull* mine = part + (u64)blockIdx.x * KMC_C_PART;
        c_block_add<true>(n_keep, ws, mine + 0);
        c_block_add<true>(n_tip, ws, mine + 1);
        c_block_add<true>(n_isl, ws, mine + 2);
        c_block_add<true>(sum, ws, mine + 3);
        c_block_add<true>(n_bad, ws, mine + 4);
        c_block_add<true>(n_bub, ws, mine + 5);
        c_block_add<true>(sum_bub, ws, mine + 6);
    } else {
        c_block_add(n_keep, ws, &ctl[KMC_C_SUM + 3]);
        c_block_add(n_tip, ws, &ctl[KMC_C_SUM + 4]);
        c_block_add(n_isl, ws, &ctl[KMC_C_SUM + 5]);
        c_block_add(sum, ws, &ctl[KMC_C_SUM + 7]);
        c_block_add(n_bad, ws, &ctl[KMC_C_BAD]);
    }
}

// Behind mark<true>, a workgroup per word of a slot (KMC_C_PART_USED of them): that word of the n_wg slots of part[] added
// up into its control word, seven atomics in all.
#define KMC_C_PART_USED 7
__global__ __launch_bounds__(KMC_C_THREADS)
void kmc_clean_reduce_kernel(const kmc_ull* __restrict__ part, u32 n_wg, kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull ws[KMC_C_WAVES];
    // a slot's words: keys kept, of tips, of islands, the kept counts, range violations, keys of bubbles, their counts
    const u32 j = blockIdx.x;
    const int word = j == 0 ? KMC_C_SUM + 3 : j == 1 ? KMC_C_SUM + 4 : j == 2 ? KMC_C_SUM + 5 : j == 3 ? KMC_C_SUM + 7 : j == 4 ? KMC_C_BAD
                   : j == 5 ? KMC_C_SUM2 + 1 : KMC_C_SUM2 + 3;
    if (j >= KMC_C_PART_USED) return;
    u64 v = 0;
    for (u32 i = threadIdx.x; i < n_wg; i += KMC_C_THREADS) v += part[(u64)i * KMC_C_PART + j];
    c_block_add(v, ws, &ctl[word]);
}

// The scatter pass, a workgroup per tile: tile_base[t] = exclusive prefix of tile_cnt; the kept rows' (hi, lo, cnt) into
// the result of n_kept entries.
template <int KW>
__global__ __launch_bounds__(KMC_C_THREADS)
void kmc_clean_scatter_kernel(const u64* __restrict__ khi, const u64* __restrict__ klo, const u64* __restrict__ cnt, u64 n,
                              const uint8_t* __restrict__ row_class, const u32* __restrict__ tile_base, u64 n_kept,
                              u64* __restrict__ ohi, u64* __restrict__ olo, u64* __restrict__ ocnt, kmc_ull* __restrict__ ctl) {
    __shared__ u32 wk[KMC_C_ROUNDS * KMC_C_WAVES];
    const u32 tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 t0 = (u64)blockIdx.x * KMC_C_TILE;
    kmc_ull m[KMC_C_ROUNDS];
#pragma unroll
    for (int r = 0; r < KMC_C_ROUNDS; ++r) {
        const u64 e = t0 + (u64)r * KMC_C_THREADS + tid;
        m[r] = __ballot(e < n && row_class[e] == KMC_CLEAN_KEEP);
        if (lane == 0) wk[r * KMC_C_WAVES + wv] = (u32)__popcll(m[r]);
    }
    __syncthreads();
    u64 pos = tile_base[blockIdx.x];
    u32 n_bad = 0;
#pragma unroll
    for (int r = 0; r < KMC_C_ROUNDS; ++r) {
        for (u32 q = 0; q < wv; ++q) pos += wk[r * KMC_C_WAVES + q];            // the earlier waves of this round
        if ((m[r] >> lane) & 1ull) {
            const u64 e = t0 + (u64)r * KMC_C_THREADS + tid;
            const u64 o = pos + __builtin_amdgcn_mbcnt_hi((u32)(m[r] >> 32), __builtin_amdgcn_mbcnt_lo((u32)m[r], 0u));
            if (o < n_kept) {
                olo[o] = klo[e];
                ocnt[o] = cnt[e];
                if (KW == 2) ohi[o] = khi[e];
            } else ++n_bad;
        }
        for (u32 q = wv; q < KMC_C_WAVES; ++q) pos += wk[r * KMC_C_WAVES + q];   // this wave and the later ones
    }
    if (n_bad) atomicAdd(&ctl[KMC_C_BAD], (kmc_ull)n_bad);
}
