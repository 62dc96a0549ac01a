// kmc_transits.hip.h -- read walks counted per graph element (include/kmc.h: kmc_unitig_transits, kmc_unitig_transits_device):
// how many reads of a batch walk each link record, which way into a unitig goes with which way out, and a verdict per
// unitig that has several of both.
//
// What a links call and a map call leave on the device is all this needs: link_offsets / link_to, segs / seg_offsets.
//   CROSSING     segment i of read r, i > seg_offsets[r], with segs[i].start == segs[i-1].start + segs[i-1].len
//                (kmc_unitig_map's definition).  start is relative to the read, so the test alone is not enough across a
//                read boundary: the first segment of a read is never a crossing.  With uni_a of segment i-1 and uni_b of
//                segment i the read leaves end a = uni_a ^ 1 and enters end b = uni_b.
//   LINK SUPPORT link_support[j] of record j = (e -> t): crossings with (a, b) == (e, t), plus, if t != e, those with
//                (a, b) == (t, e) -- the same link read on the other strand.  One end never has two records with one target
//                (distinct extension bases reach distinct keys, hence distinct ends), so "the record e -> t" is one index.
//                A crossing for which neither a -> b nor b -> a is a record is counted in the summary and nowhere else.
//   TRANSIT      segment i such that i and i + 1 are both crossings of one read: the read came from end a, ran through
//                unitig v = uni_i >> 1 (o = uni_i & 1: e_in = 2v + o, e_out = 2v + 1 - o) and enters end b' next.  p is the
//                rank of the record e_in -> a among those of e_in, q the rank of e_out -> b' among those of e_out; if
//                either record is missing the transit is dropped and counted.  Stored orientation-free: (P, Q) = (p, q) if
//                o == 0, else (q, p) -- P a rank at the START end 2v, Q one at the END end 2v + 1.
//   MATRIX       with dS / dE the record counts of ends 2v / 2v + 1: transit_offsets[v + 1] - transit_offsets[v] == dS * dE,
//                slot transit_offsets[v] + P * dE + Q.  Dense, at most 16 slots per unitig, zeros stored: no sort, no hash.
//   VERDICT      PLAIN iff dS < 2 or dE < 2.  Otherwise a slot is supported iff its count >= min_reads; UNSPANNED: none is;
//                RESOLVED: every row and every column holds exactly one supported slot; AMBIGUOUS: the rest.
// Identities: summary[0] equals kmc_unitig_map's summary[4] of the batch (the host checks it on every call); the sum of
// transit_count equals [3]; where the record set is symmetric [1] == [4] == 0 and the sum of link_support equals
// 2 * [0] - (crossings with a == b).
//
// Kernels.  LAYOUT: a lane per unitig, dS * dE into a u32 that kmc_scan.hip.h scans; a second lane per unitig widens the scan
// into transit_offsets.  FIRST: a lane per read marks its first segment in a map of one BYTE per segment -- plain stores; a
// bit per segment would need an atomic OR per read, and a search of seg_offsets per segment some twenty dependent loads.
// The transit lane reads two bytes of it instead.  TRANSIT: a lane per segment; the record lookups are linear scans of at
// most four link_to entries.  COMBINE: before the atomics the lanes of a wave that hold the same target elect a leader who
// adds their number (kmc_cc_stats_kernel's loop, bounded by KMC_T_LEADERS rounds, given up if the first leader is alone; what
// is left goes alone); without it every
// lane adds 1 (DESIGN.md has both numbers).  VERDICT: a lane per unitig reads its slots into row and column masks; a lane per
// record counts the unsupported ones.
//
// No kernel waits for another workgroup and every loop is bounded by the batch, the graph or a constant.  Every index that
// comes from device data -- a unitig id, an end, a record index, a slot, a read's segment -- is compared with its array's size
// before it addresses anything; a violation is counted in ctl[KMC_T_BAD] and the host fails the call.
#pragma once
#include "kmc_links.hip.h"
#include "kmc_map.hip.h"

#define KMC_T_THREADS 256
#define KMC_T_WAVES (KMC_T_THREADS / 64)
#define KMC_T_LEADERS 16
#define KMC_T_NONE 0xFFFFFFFFFFFFFFFFull
// control words: [0..7] the summary words of this call ([0], [1], [3], [4] of this batch alone), [8] range violations,
// [9] the total of the layout scan (u32), [10] the same total as the layout kernel adds it up in 64 bits
#define KMC_T_CROSS 0
#define KMC_T_ORPHAN 1
#define KMC_T_ZERO 2
#define KMC_T_STORED 3
#define KMC_T_DROPPED 4
#define KMC_T_REPEAT 5
#define KMC_T_RESOLVED 6
#define KMC_T_AMBIG 7
#define KMC_T_BAD 8
#define KMC_T_SCAN 9
#define KMC_T_SLOTS 10
#define KMC_T_CTL_WORDS 11

struct TransitGraph {
    const u64* link_offsets;   // 2 * n_unitigs + 1
    const u32* link_to;        // n_links
    u64 n_unitigs, n_links;
};

// the records of end e (< 2 * n_unitigs): [lo, lo + d), d <= 4, inside link_to; false if the offsets say otherwise
__device__ __forceinline__ bool t_records(const TransitGraph& g, u32 e, u64& lo, u32& d) {
    lo = g.link_offsets[e];
    const u64 hi = g.link_offsets[e + 1];
    d = (u32)(hi - lo);
    return hi >= lo && hi - lo <= 4 && hi <= g.n_links;
}

// the rank of the record with target t among the d records at lo, or 4
__device__ __forceinline__ u32 t_rank(const TransitGraph& g, u64 lo, u32 d, u32 t) {
    u32 r = 4;
#pragma unroll
    for (u32 i = 0; i < 4; ++i)
        if (i < d && r == 4 && g.link_to[lo + i] == t) r = i;
    return r;
}

// slots[u] = dS(u) * dE(u); their sum in 64 bits beside the scan's u32
__global__ __launch_bounds__(KMC_T_THREADS)
void kmc_transit_layout_kernel(TransitGraph g, u32* __restrict__ slots, kmc_ull* __restrict__ ctl) {
    const u64 u = (u64)blockIdx.x * KMC_T_THREADS + threadIdx.x;
    u32 n = 0, bad = 0;
    if (u < g.n_unitigs) {
        u64 ls, le;
        u32 ds, de;
        if (t_records(g, (u32)(2 * u), ls, ds) && t_records(g, (u32)(2 * u + 1), le, de)) n = ds * de; else bad = 1;
        slots[u] = n;
    }
    const u64 sn = wave_sum_u64((u64)n), sb = wave_sum_u64((u64)bad);
    if ((threadIdx.x & 63) == 0) {
        if (sn) atomicAdd(&ctl[KMC_T_SLOTS], (kmc_ull)sn);
        if (sb) atomicAdd(&ctl[KMC_T_BAD], (kmc_ull)sb);
    }
}

// transit_offsets[u] = pos[u] as a u64, transit_offsets[n_unitigs] = n_slots
__global__ __launch_bounds__(KMC_T_THREADS)
void kmc_transit_offsets_kernel(const u32* __restrict__ pos, u64 n_unitigs, u64 n_slots, u64* __restrict__ transit_offsets) {
    const u64 u = (u64)blockIdx.x * KMC_T_THREADS + threadIdx.x;
    if (u < n_unitigs) transit_offsets[u] = pos[u];
    if (u == 0) transit_offsets[n_unitigs] = n_slots;
}

// first[seg_offsets[r]] = 1 for every read with a segment (first is zeroed before)
__global__ __launch_bounds__(KMC_T_THREADS)
void kmc_transit_first_kernel(const u64* __restrict__ seg_offsets, u64 n_reads, u64 n_segs, uint8_t* __restrict__ first,
                              kmc_ull* __restrict__ ctl) {
    const u64 r = (u64)blockIdx.x * KMC_T_THREADS + threadIdx.x;
    bool bad = false;
    if (r < n_reads) {
        const u64 a = seg_offsets[r], b = seg_offsets[r + 1];
        if (a > b || b > n_segs) bad = true;
        else if (a < b) first[a] = 1;
    }
    const u64 m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[KMC_T_BAD], (kmc_ull)__popcll(m));
}

// dst[at] += 1 for every lane with at != KMC_T_NONE; COMBINE: one atomic per distinct `at` of the wave for the first
// KMC_T_LEADERS of them -- unless the first leader turns out to be alone with its target, the sign of a wave whose targets
// are mostly different, where the rounds would find nothing to combine.  Every lane of the wave calls it.
template <bool COMBINE>
__device__ __forceinline__ void t_add(kmc_ull* __restrict__ dst, u64 at, int lane) {
    bool mine = at != KMC_T_NONE;
    if (COMBINE) {
        kmc_ull left = __builtin_amdgcn_ballot_w64(mine);
        for (int it = 0; it < KMC_T_LEADERS && left; ++it) {   // (wave-uniform: left and who come from ballots alone)
            const int leader = __builtin_ctzll(left);
            const u64 al = __shfl(at, leader);
            const bool same = mine && at == al;
            const kmc_ull who = __builtin_amdgcn_ballot_w64(same);
            if (lane == leader) atomicAdd(dst + al, (kmc_ull)__popcll(who));
            if (same) mine = false;
            left &= ~who;
            if (it == 0 && (who & (who - 1)) == 0) break;
        }
    }
    if (mine) atomicAdd(dst + at, 1ull);
}

// A lane per segment: the crossing into it, the transit through it
template <bool COMBINE>
__global__ __launch_bounds__(KMC_T_THREADS)
void kmc_transit_kernel(TransitGraph g, const uint4* __restrict__ segs, const uint8_t* __restrict__ first, u64 n_segs,
                        const u64* __restrict__ transit_offsets, u64 n_slots, kmc_ull* __restrict__ link_support,
                        kmc_ull* __restrict__ transit_count, kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull part[KMC_T_WAVES][5];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 stride = (u64)gridDim.x * KMC_T_THREADS;
    const u64 rounds = (n_segs + stride - 1) / stride;   // the same for every lane: t_add is called by whole waves
    u64 n_cross = 0, n_orphan = 0, n_stored = 0, n_dropped = 0, n_bad = 0;
    for (u64 it = 0; it < rounds; ++it) {
        const u64 i = it * stride + (u64)blockIdx.x * KMC_T_THREADS + tid;
        u64 at_ab = KMC_T_NONE, at_ba = KMC_T_NONE, at_slot = KMC_T_NONE;
        if (i < n_segs && i > 0 && !first[i]) {
            const uint4 s = segs[i], p = segs[i - 1];
            const u32 a = p.z ^ 1u, b = s.z;
            if (s.x == p.x + p.y) {
                if ((u64)(a >> 1) >= g.n_unitigs || (u64)(b >> 1) >= g.n_unitigs) ++n_bad;
                else {
                    u64 la, lb;
                    u32 da, db;
                    if (!t_records(g, a, la, da) || !t_records(g, b, lb, db)) ++n_bad;
                    else {
                        ++n_cross;
                        const u32 r_ab = t_rank(g, la, da, b), r_ba = t_rank(g, lb, db, a);   // (a == b: one and the same record)
                        if (r_ab < 4) at_ab = la + r_ab;
                        if (r_ba < 4 && a != b) at_ba = lb + r_ba;
                        if (r_ab == 4 && r_ba == 4) ++n_orphan;
                        // the transit through segment i: the read goes on into segment i + 1 without a gap
                        if (i + 1 < n_segs && !first[i + 1]) {
                            const uint4 nx = segs[i + 1];
                            if (nx.x == s.x + s.y) {
                                const u32 e_out = b ^ 1u, v = b >> 1, o = b & 1u;
                                u64 lo_out;
                                u32 d_out;
                                if ((u64)(nx.z >> 1) >= g.n_unitigs || !t_records(g, e_out, lo_out, d_out)) ++n_bad;
                                else {
                                    const u32 q = t_rank(g, lo_out, d_out, nx.z);   // (p is r_ba: e_in == b)
                                    if (r_ba == 4 || q == 4) ++n_dropped;
                                    else {
                                        const u32 P = o ? q : r_ba, Q = o ? r_ba : q, dS = o ? d_out : db, dE = o ? db : d_out;
                                        const u64 slot = transit_offsets[v] + (u64)P * dE + Q;
                                        if (P >= dS || Q >= dE || slot >= n_slots) ++n_bad;
                                        else { at_slot = slot; ++n_stored; }
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        t_add<COMBINE>(link_support, at_ab, lane);
        t_add<COMBINE>(link_support, at_ba, lane);
        t_add<COMBINE>(transit_count, at_slot, lane);
    }
    // totals: one atomic per workgroup and word
    const u64 s0 = wave_sum_u64(n_cross), s1 = wave_sum_u64(n_orphan), s2 = wave_sum_u64(n_stored), s3 = wave_sum_u64(n_dropped),
              s4 = wave_sum_u64(n_bad);
    if (lane == 0) { part[wv][0] = s0; part[wv][1] = s1; part[wv][2] = s2; part[wv][3] = s3; part[wv][4] = s4; }
    __syncthreads();
    if (tid < 5) {
        kmc_ull s = 0;
#pragma unroll
        for (int w = 0; w < KMC_T_WAVES; ++w) s += part[w][tid];
        const int word = tid == 0 ? KMC_T_CROSS : tid == 1 ? KMC_T_ORPHAN : tid == 2 ? KMC_T_STORED : tid == 3 ? KMC_T_DROPPED : KMC_T_BAD;
        if (s) atomicAdd(&ctl[word], s);
    }
}

// Lane x < n_unitigs: verdict[x] from the slots of unitig x; lane x < n_links: is record x unsupported
__global__ __launch_bounds__(KMC_T_THREADS)
void kmc_transit_verdict_kernel(TransitGraph g, const u64* __restrict__ transit_offsets, u64 n_slots, const kmc_ull* __restrict__ link_support,
                                const kmc_ull* __restrict__ transit_count, u64 min_reads, uint8_t* __restrict__ verdict,
                                kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull part[KMC_T_WAVES][5];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 x = (u64)blockIdx.x * KMC_T_THREADS + tid;
    u32 zero = 0, repeat = 0, resolved = 0, ambig = 0, bad = 0;
    if (x < g.n_links) zero = link_support[x] == 0 ? 1u : 0u;
    if (x < g.n_unitigs) {
        u64 ls, le;
        u32 ds = 0, de = 0, vd = KMC_TRANSIT_PLAIN;
        const u64 t0 = transit_offsets[x], t1 = transit_offsets[x + 1];
        if (!t_records(g, (u32)(2 * x), ls, ds) || !t_records(g, (u32)(2 * x + 1), le, de) || t1 < t0 || t1 - t0 != (u64)ds * de || t1 > n_slots) bad = 1;
        else if (ds >= 2 && de >= 2) {
            u32 row1 = 0, row2 = 0, col1 = 0, col2 = 0;   // bit P / Q: the row / column holds one supported slot at least / two at least
#pragma unroll
            for (u32 P = 0; P < 4; ++P)
#pragma unroll
                for (u32 Q = 0; Q < 4; ++Q)
                    if (P < ds && Q < de && transit_count[t0 + P * de + Q] >= min_reads) {
                        row2 |= row1 & (1u << P); row1 |= 1u << P;
                        col2 |= col1 & (1u << Q); col1 |= 1u << Q;
                    }
            repeat = 1;
            if (!row1) vd = KMC_TRANSIT_UNSPANNED;
            else if (row1 == (1u << ds) - 1u && col1 == (1u << de) - 1u && !row2 && !col2) { vd = KMC_TRANSIT_RESOLVED; resolved = 1; }
            else { vd = KMC_TRANSIT_AMBIGUOUS; ambig = 1; }
        }
        verdict[x] = (uint8_t)vd;
    }
    const u64 s0 = wave_sum_u64((u64)zero), s1 = wave_sum_u64((u64)repeat), s2 = wave_sum_u64((u64)resolved), s3 = wave_sum_u64((u64)ambig),
              s4 = wave_sum_u64((u64)bad);
    if (lane == 0) { part[wv][0] = s0; part[wv][1] = s1; part[wv][2] = s2; part[wv][3] = s3; part[wv][4] = s4; }
    __syncthreads();
    if (tid < 5) {
        kmc_ull s = 0;
#pragma unroll
        for (int w = 0; w < KMC_T_WAVES; ++w) s += part[w][tid];
        const int word = tid == 0 ? KMC_T_ZERO : tid == 1 ? KMC_T_REPEAT : tid == 2 ? KMC_T_RESOLVED : tid == 3 ? KMC_T_AMBIG : KMC_T_BAD;
        if (s) atomicAdd(&ctl[word], s);
    }
}
