// kmc_bubbles.hip.h -- the bubbles of the compacted graph reported as variant records (include/kmc.h: kmc_unitig_bubbles,
// kmc_unitig_bubbles_device): for every bubble arm that loses against a parallel arm, the pair, the two ends it sits between
// and how the two spellings differ.
//
// What a links call leaves on the device is all this needs: the unitig arrays (bases, offsets, abund, flags) and the link
// records (link_offsets per end, link_to).  The candidate rule, the ends of a candidate and the order "w beats u" are those of
// kmc_clean.hip.h (c_unit, c_bubble_ends, c_beats), used from there.
//   pair      a lane per unitig, the shape of the simplify verdict kernel.  A candidate follows the one record of its START
//             end, walks the at most four records of the end it reaches and keeps the greatest of the candidates parallel to
//             it; it is called iff that one beats it.  Per unitig a flag word and major(u); the totals go through a wave
//             sum before an atomic.
//   (scan)    kmc_scan.hip.h over the flags: a record's slot is the number of called unitigs before it, so the records come
//             out in ascending u.
//   place     a lane per unitig: a called one writes u, w, p, q into its slot.
//   diff      a wave per record.  Lane i holds position i of U and of the oriented W (read from the far end and complemented
//             for a reversed arm), 64 positions a step; the ballot of the unequal lanes gives lcp from its lowest bit and adds
//             its popcount to mism.  A second sweep from the far ends gives lcs under the cap min(|U|, |W|) - lcp.  Every
//             loop bound is uniform over the wave: no lane walks bytes on its own.  A wave takes records r, r + waves, ...
//             and a workgroup adds its totals once at the end.
//
// No kernel waits for another workgroup and every loop is bounded by the unitigs, the records, an arm's length or constants.
// Every index that comes from device data -- a record's position and target end, a sibling end, a unitig id, a slot, a base
// position -- is compared with its array's size before it addresses anything; a violation is counted in ctl[KMC_B_BAD] and
// the host fails the call.
#pragma once
#include "kmc_clean.hip.h"

#define KMC_B_THREADS 256
#define KMC_B_WAVES (KMC_B_THREADS / 64)
#define KMC_B_REC 8        // KMC_BUBBLE_RECORD_WORDS
// control words: [0] the total of the scan (u32), then candidates, called, the keys of the called arms, substitutions,
// indels, complex, reversed, range violations
#define KMC_B_CAND 1
#define KMC_B_CALLED 2
#define KMC_B_KEYS 3
#define KMC_B_SUBST 4
#define KMC_B_INDEL 5
#define KMC_B_COMPLEX 6
#define KMC_B_REVERSED 7
#define KMC_B_BAD 8
#define KMC_B_CTL_WORDS 9

// flag[u] = 1 iff u is called, major[u] = major(u) then (0 otherwise); g.max_bubble is the candidate limit
__global__ __launch_bounds__(KMC_B_THREADS)
void kmc_bubble_pair_kernel(CleanGraph g, u32* __restrict__ flag, u32* __restrict__ major, kmc_ull* __restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    const u64 u = (u64)blockIdx.x * KMC_B_THREADS + threadIdx.x;
    const u64 n_ends = 2 * g.n_unitigs;
    u32 cand = 0, called = 0, bad = 0;
    u64 keys = 0;
    if (u < g.n_unitigs) {
        const CUnit me = c_unit(g, u);
        u64 best = 0;
        if (!me.circ && me.r0 == 1 && me.r1 == 1 && me.m <= g.max_bubble) {
            u64 p = 0, q = 0;
            if (c_bubble_ends(g, me, u, n_ends, &p, &q, &bad)) {
                cand = 1;
                const u64 s0 = g.link_offsets[p], s1 = g.link_offsets[p + 1];
                if (s1 < s0 || s1 - s0 > 4 || s1 > g.n_links) {
                    ++bad;
                } else {
                    bool have = false;
                    CUnit top = me;
                    for (u64 i = s0; i < s1; ++i) {   // (at most four)
                        const u64 s = g.link_to[i];
                        if (s >= n_ends) { ++bad; continue; }
                        const u64 w = s >> 1;
                        if (w == u) continue;
                        const CUnit sib = c_unit(g, w);
                        if (sib.circ || sib.r0 != 1 || sib.r1 != 1 || sib.m > g.max_bubble) continue;
                        u64 wp = 0, wq = 0;
                        if (!c_bubble_ends(g, sib, w, n_ends, &wp, &wq, &bad)) continue;
                        if (!((wp == p && wq == q) || (wp == q && wq == p))) continue;
                        if (!have || c_beats(sib, w, top, best)) { have = true; best = w; top = sib; }
                    }
                    if (have && c_beats(top, best, me, u)) { called = 1; keys = me.m; }
                }
            }
        }
        flag[u] = called;
        major[u] = called ? (u32)best : 0u;
    }
    const u64 sc = wave_sum_u64((u64)cand), sp = wave_sum_u64((u64)called), sk = wave_sum_u64(keys), sb = wave_sum_u64((u64)bad);
    if (lane == 0) {
        if (sc) atomicAdd(&ctl[KMC_B_CAND], (kmc_ull)sc);
        if (sp) atomicAdd(&ctl[KMC_B_CALLED], (kmc_ull)sp);
        if (sk) atomicAdd(&ctl[KMC_B_KEYS], (kmc_ull)sk);
        if (sb) atomicAdd(&ctl[KMC_B_BAD], (kmc_ull)sb);
    }
}

// Behind the exclusive scan of flag[] into pos[]: words 0..3 of the record of every called unitig.  p and q are read again
// from the one record at each of u's ends (the pair kernel found both inside their arrays; they are checked as there).
__global__ __launch_bounds__(KMC_B_THREADS)
void kmc_bubble_place_kernel(CleanGraph g, const u32* __restrict__ flag, const u32* __restrict__ pos, const u32* __restrict__ major,
                             u64 n_records, u32* __restrict__ rec, kmc_ull* __restrict__ ctl) {
    const u64 u = (u64)blockIdx.x * KMC_B_THREADS + threadIdx.x;
    if (u >= g.n_unitigs || !flag[u]) return;
    const u64 r = pos[u], o0 = g.link_offsets[2 * u], o1 = g.link_offsets[2 * u + 1];
    if (r >= n_records || o0 >= g.n_links || o1 >= g.n_links) { atomicAdd(&ctl[KMC_B_BAD], (kmc_ull)1); return; }
    u32* out = rec + r * KMC_B_REC;
    out[0] = (u32)u;
    out[1] = major[u];
    out[2] = g.link_to[o0];
    out[3] = g.link_to[o1];
}

__device__ __forceinline__ uint8_t b_complement(uint8_t c) {
    return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
}

// Position i of the oriented arm whose spelling is the len bases at s: the spelling itself, or its reverse complement
__device__ __forceinline__ uint8_t b_at(const uint8_t* __restrict__ s, u32 len, u32 i, bool reversed) {
    return reversed ? b_complement(s[len - 1 - i]) : s[i];
}

// Words 4..7 of every record; ctl[KMC_B_SUBST ..] the totals.  bases has n_bases bytes.
__global__ __launch_bounds__(KMC_B_THREADS)
void kmc_bubble_diff_kernel(CleanGraph g, const uint8_t* __restrict__ bases, u64 n_bases, u64 n_records, u32* __restrict__ rec,
                            kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull ws[KMC_B_WAVES];
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 n_waves = (u64)gridDim.x * KMC_B_WAVES;
    u32 n_subst = 0, n_indel = 0, n_complex = 0, n_rev = 0, n_bad = 0;   // (the same in every lane of a wave)
    for (u64 r = (u64)blockIdx.x * KMC_B_WAVES + wv; r < n_records; r += n_waves) {
        u32* out = rec + r * KMC_B_REC;
        const u64 u = out[0], w = out[1], p = out[2];
        if (u >= g.n_unitigs || w >= g.n_unitigs) { ++n_bad; continue; }
        const u64 ub = g.offsets[u], ue = g.offsets[u + 1], wb = g.offsets[w], we = g.offsets[w + 1], ws0 = g.link_offsets[2 * w];
        if (ue < ub || we < wb || ue > n_bases || we > n_bases || ue - ub > 0xFFFFFFFFull || we - wb > 0xFFFFFFFFull || ws0 >= g.n_links) {
            ++n_bad;
            continue;
        }
        const u32 lu = (u32)(ue - ub), lw = (u32)(we - wb), n = lu < lw ? lu : lw;
        const bool reversed = (u64)g.link_to[ws0] != p;
        const uint8_t* su = bases + ub;
        const uint8_t* sw = bases + wb;
        // from the front: lcp, and over arms of one length every unequal position
        u32 lcp = n, mism = 0;
        bool found = false;
        for (u32 i0 = 0; i0 < n && (lu == lw || !found); i0 += 64) {
            const u32 i = i0 + lane;
            const bool ne = i < n && su[i] != b_at(sw, lw, i, reversed);
            const kmc_ull mask = __ballot(ne);
            if (mask && !found) { found = true; lcp = i0 + (u32)__builtin_ctzll(mask); }
            mism += (u32)__popcll(mask);
        }
        if (lu != lw) mism = 0;
        // from the back, over what the prefix left of the shorter arm
        const u32 cap = n - lcp;
        u32 lcs = cap;
        found = false;
        for (u32 j0 = 0; j0 < cap && !found; j0 += 64) {
            const u32 j = j0 + lane;
            const bool ne = j < cap && su[lu - 1 - j] != b_at(sw, lw, lw - 1 - j, reversed);
            const kmc_ull mask = __ballot(ne);
            if (mask) { found = true; lcs = j0 + (u32)__builtin_ctzll(mask); }
        }
        const u32 au = lu - lcp - lcs, aw = lw - lcp - lcs;
        const u32 kind = (lu == lw && mism == 1) ? KMC_BUBBLE_SUBST : ((au == 0) != (aw == 0)) ? KMC_BUBBLE_INDEL : KMC_BUBBLE_COMPLEX;
        n_subst += kind == KMC_BUBBLE_SUBST;
        n_indel += kind == KMC_BUBBLE_INDEL;
        n_complex += kind == KMC_BUBBLE_COMPLEX;
        n_rev += reversed ? 1u : 0u;
        if (lane == 0) {
            out[4] = lcp;
            out[5] = lcs;
            out[6] = kind | (reversed ? KMC_BUBBLE_REVERSED : 0u);
            out[7] = mism;
        }
    }
    // a wave's totals sit in each of its lanes: lane 0 hands them on, thread 0 adds the workgroup's
    const u32 part[5] = {n_subst, n_indel, n_complex, n_rev, n_bad};
    const int word[5] = {KMC_B_SUBST, KMC_B_INDEL, KMC_B_COMPLEX, KMC_B_REVERSED, KMC_B_BAD};
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        __syncthreads();
        if (lane == 0) ws[wv] = part[t];
        __syncthreads();
        if (threadIdx.x == 0) {
            kmc_ull s = 0;
            for (int q = 0; q < KMC_B_WAVES; ++q) s += ws[q];
            if (s) atomicAdd(&ctl[word[t]], s);
        }
    }
}
