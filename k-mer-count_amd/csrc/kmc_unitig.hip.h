// kmc_unitig.hip.h -- the unitigs of the de Bruijn graph of the sorted view (include/kmc.h: kmc_unitigs, kmc_unitigs_device):
// the maximal non-branching paths spelled out, on top of the adj words of kmc_graph.hip.h.
//
// A SIDE STATE is a = 2 * row + s (s = 0: side R, 1: side L) of a view row; a ^ 1 is the other side of the same key.
//   link[a]    the side state that faces a across its one edge, if side a continues in adj (KMC_U_NONE otherwise)
//   joined[a]  link[a] if the two sides name each other and are not the same side (the mutual rule), KMC_U_NONE otherwise.
//              Joins are a symmetric matching, so the keys fall into simple paths and simple cycles.
//   ranking    next(a) = joined[a] ^ 1 (cross the edge, cross the key); a terminal (not joined) is its own end at distance 0.
//              Pointer doubling over the 2n states, double-buffered, one launch per round.  Every round counts the states
//              whose pointer is not a terminal yet; while a path state is unfinished that count falls strictly (a path that
//              holds a state 2^t + x hops from its end holds one 2^(t-1) + 1 hops from it), so the first round that repeats
//              its predecessor's count has finished every path, and what it still counts are the states on cycles.  The
//              host looks at the counts every few rounds and never launches more than ceil(log2(2n)) + 1: no kernel waits
//              for another workgroup, and termination comes from that bound, not from the data.
//   cycles     (only when that count is not 0) a min-row doubling along next() -- ceil(log2(cycle states)) rounds cover
//              the longest cycle -- then the thread that owns side L of a cycle's smallest row cuts its join, marks the key,
//              and the ranking runs again.
//   layout     a key knows the end keys and distances on both of its sides: from them the first key of its unitig, its
//              position and its reading sense.  First keys are flagged and scanned (unitig ids), their key counts are
//              scanned (key offsets); both scans run over the view rows, so neither needs the number of unitigs.
//   emit       a lane per key writes its one base (a first key its k), adds its count to abund[id]; first keys write
//              offsets / flags and feed the summary words, which a wave keeps in registers until its last trip.
#pragma once
#include "kmc_graph.hip.h"

#define KMC_U_THREADS 256
#define KMC_U_WAVES (KMC_U_THREADS / 64)
#define KMC_U_NONE KMC_Q_NOPOS
#define KMC_U_WORDS 8         // KMC_UNITIG_WORDS
#define KMC_U_ROUND_SLOTS 40  // not-finished counts: slot 0 the initial states, slot t round t (at most 33 rounds)
#define KMC_U_CYC 2u          // circ[row]: the key lies on a cycle (bit 1), it is the key its cycle was cut at (bit 0)

// link[2i], link[2i + 1] of view row i.  A side that continues has degree 1, so its one neighbour is the set bit of its
// nibble; the neighbour key and its strand come from the arithmetic of kmc_graph_kernel's first round.
template <int KW, bool CANON>
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_link_kernel(QView v, int k, const uint16_t* __restrict__ adj, u32* __restrict__ link) {
    const u64 i = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    const bool act = i < v.n;
    const int tb = 2 * k - 2;
    u32 a = 0;
    u64 xlo = 0, xhi = 0;
    if (act) {
        a = adj[i];
        xlo = v.lo[i];
        if (KW == 2) xhi = v.hi[i];
    }
    const bool go_r = act && (a >> 10 & 1) && !(a >> 8 & 1), go_l = act && (a >> 10 & 1) && !(a >> 9 & 1);
    const u64 cr = go_r ? (u64)(__ffs(a & 15u) - 1) : 0ull, cl = go_l ? (u64)(__ffs((a >> 4) & 15u) - 1) : 0ull;
    u64 khi[2], klo[2];
    u32 face[2];   // the side of the neighbour that faces back
    g_shl2<KW>(xhi, xlo, v.max_hi, v.max_lo, khi[0], klo[0]);   // x[1:] + c: kept -> entered on L
    klo[0] |= cr;
    g_shr2<KW>(xhi, xlo, khi[1], klo[1]);                       // c + x[:-1]: kept -> entered on R
    g_top_or<KW>(khi[1], klo[1], tb, cl);
    face[0] = 1u; face[1] = 0u;
    if (CANON) {
        u64 rhi, rlo, qhi, qlo, phi, plo;
        revcomp_key(xhi, xlo, k, rhi, rlo);
        g_shr2<KW>(rhi, rlo, qhi, qlo);                         // revcomp(x[1:] + c) = comp(c) + revcomp(x)[:-1]
        g_top_or<KW>(qhi, qlo, tb, 3ull - cr);
        if (key_less(qhi, qlo, khi[0], klo[0])) { khi[0] = qhi; klo[0] = qlo; face[0] = 0u; }
        g_shl2<KW>(rhi, rlo, v.max_hi, v.max_lo, phi, plo);     // revcomp(c + x[:-1]) = revcomp(x)[1:] + comp(c)
        plo |= 3ull - cl;
        if (key_less(phi, plo, khi[1], klo[1])) { khi[1] = phi; klo[1] = plo; face[1] = 1u; }
    }
    u32 pos[2];
    q_find<KW, 2>(v, khi, klo, (go_r ? 1u : 0u) | (go_l ? 2u : 0u), pos);
    if (act) {
        uint2 o;
        o.x = pos[0] == KMC_U_NONE ? KMC_U_NONE : 2u * pos[0] + face[0];
        o.y = pos[1] == KMC_U_NONE ? KMC_U_NONE : 2u * pos[1] + face[1];
        reinterpret_cast<uint2*>(link)[i] = o;
    }
}

// the sum of a per-lane flag over the wave into *ctr (one atomic per wave, none if the sum is 0)
__device__ __forceinline__ void u_wave_count(bool flag, u32* ctr) {
    const u64 m = __builtin_amdgcn_ballot_w64(flag);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(ctr, (u32)__popcll(m));
}

// joined[a] by the mutual rule, from link alone (a separate array: the result does not depend on scheduling);
// *unjoined counts the sides that continue in adj and are not joined
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_join_kernel(const u32* __restrict__ link, u64 n2, u32* __restrict__ joined, kmc_ull* __restrict__ unjoined) {
    const u64 a = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    bool lost = false;
    if (a < n2) {
        const u32 b = link[a];
        u32 j = KMC_U_NONE;
        if (b != KMC_U_NONE) {
            if (b != (u32)a && link[b] == (u32)a) j = b; else lost = true;
        }
        joined[a] = j;
    }
    const u64 m = __builtin_amdgcn_ballot_w64(lost);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(unjoined, (kmc_ull)__popcll(m));
}

// ranking, round 0: a terminal points at itself, every other state one hop on.  cnt[0] = the states that are not terminals
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_rank_init_kernel(const u32* __restrict__ joined, u64 n2, u32* __restrict__ ptr, u32* __restrict__ dist,
                                 u32* __restrict__ cnt) {
    const u64 a = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    bool open = false;
    if (a < n2) {
        const u32 j = joined[a];
        open = j != KMC_U_NONE;
        ptr[a] = open ? j ^ 1u : (u32)a;
        dist[a] = open ? 1u : 0u;
    }
    u_wave_count(open, cnt);
}

// one doubling round from (ptr, dist) into (ptr2, dist2).  *cnt = the states whose pointer was not a terminal BEFORE this
// round (slot t counts the states more than 2^(t-1) hops from their end, and those on cycles).  A fixed point p of ptr is
// a terminal, or a state of a cycle whose length divides the hops covered so far; then every state of that cycle points
// at itself, so a fixed point reached from ANOTHER state is a terminal, and a state that points at itself asks joined.
// (dist of a state on a cycle wraps; it is never used.)
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_rank_round_kernel(const u32* __restrict__ joined, u64 n2, const u32* __restrict__ ptr, const u32* __restrict__ dist,
                                  u32* __restrict__ ptr2, u32* __restrict__ dist2, u32* __restrict__ cnt) {
    const u64 a = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    bool open = false;
    if (a < n2) {
        const u32 p = ptr[a], d = dist[a];
        const u32 q = ptr[p], dq = dist[p];
        ptr2[a] = q;
        dist2[a] = d + dq;
        open = q != p;   // q == p: p is a fixed point, so q is too
        if (!open && q == (u32)a) open = joined[a] != KMC_U_NONE;
    }
    u_wave_count(open, cnt);
}

// circ[row] = KMC_U_CYC iff the key lies on a cycle: the ranking left the pointer of its side L on a state that is joined
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_cycle_mark_kernel(const u32* __restrict__ joined, const u32* __restrict__ ptr, u64 n, uint8_t* __restrict__ circ) {
    const u64 r = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    if (r < n) circ[r] = joined[ptr[2 * r + 1]] != KMC_U_NONE ? (uint8_t)KMC_U_CYC : (uint8_t)0;
}

// the smallest row along next(): start and one doubling round (every state takes part; only those on cycles are used)
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_minrow_init_kernel(const u32* __restrict__ joined, u64 n2, u32* __restrict__ ptr, u32* __restrict__ mrow) {
    const u64 a = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    if (a < n2) {
        const u32 j = joined[a];
        ptr[a] = j != KMC_U_NONE ? j ^ 1u : (u32)a;
        mrow[a] = (u32)(a >> 1);
    }
}
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_minrow_round_kernel(u64 n2, const u32* __restrict__ ptr, const u32* __restrict__ mrow, u32* __restrict__ ptr2,
                                    u32* __restrict__ mrow2) {
    const u64 a = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    if (a < n2) {
        const u32 p = ptr[a];
        const u32 m = mrow[a], mp = mrow[p];
        ptr2[a] = ptr[p];
        mrow2[a] = mp < m ? mp : m;
    }
}

// The cut: the thread of the row that is its cycle's smallest takes the join of its side L apart, both ends, and marks the
// key.  No other thread of this launch reads or writes those two entries: a thread reads joined only for a row that is
// its cycle's smallest, and a cycle has one.
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_cycle_cut_kernel(const u32* __restrict__ mrow, u64 n, u32* __restrict__ joined, uint8_t* __restrict__ circ) {
    const u64 r = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    if (r >= n || circ[r] != KMC_U_CYC) return;
    const u64 a = 2 * r + 1;
    if (mrow[a] != (u32)r) return;
    const u32 b = joined[a];
    joined[a] = KMC_U_NONE;
    if (b != KMC_U_NONE) joined[b] = KMC_U_NONE;
    circ[r] = (uint8_t)(KMC_U_CYC | 1u);
}

// Where a solid key stands in its unitig: the row of the unitig's first key, its own position, the unitig's keys, and
// whether it is read on its other strand.  Side R leads to end key e.x at distance d.x, side L to e.y at d.y.  The reading
// starts at the end key of the smaller row; in a forward ctx, and for a one-key unitig, at the one whose L side ends it.
struct UPlace { u32 first, pos, len; bool rc; };
__device__ __forceinline__ UPlace u_place(u64 r, const u32* __restrict__ ptr, const u32* __restrict__ dist, bool canon) {
    const uint2 e = reinterpret_cast<const uint2*>(ptr)[r], d = reinterpret_cast<const uint2*>(dist)[r];
    const u32 er = e.x >> 1, el = e.y >> 1;
    UPlace p;
    p.rc = canon && er < el;
    p.first = p.rc ? er : el;
    p.pos = p.rc ? d.x : d.y;
    p.len = d.x + d.y + 1u;
    return p;
}

// per view row: is it the first key of a unitig, and if so of how many keys (0 otherwise): the inputs of the two scans
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_place_kernel(u64 n, const uint16_t* __restrict__ adj, const u32* __restrict__ ptr, const u32* __restrict__ dist,
                             int canon, u32* __restrict__ is_first, u32* __restrict__ first_len) {
    const u64 r = (u64)blockIdx.x * KMC_U_THREADS + threadIdx.x;
    if (r >= n) return;
    u32 f = 0, l = 0;
    if (adj[r] >> 10 & 1) {
        const UPlace p = u_place(r, ptr, dist, canon != 0);
        if (p.pos == 0) { f = 1; l = p.len; }
    }
    is_first[r] = f;
    first_len[r] = l;
}

__device__ __forceinline__ uint8_t u_ascii(u32 code) { return (uint8_t)(0x54474341u >> (8 * code)); }   // "ACGT"[code]

// uid_of / koff_of: the exclusive scans of is_first / first_len.  abund is zero before the launch; summary[3], [4], [5], [7]
// are accumulated here (circular, one-key, keys of the longest, sum of abund).  offsets[n_unitigs] = n_bases.  summary[0]
// is zero before the launch and counts the solid keys whose place falls outside the output: the layout covers every solid
// key, so the host takes anything but 0 for an internal error instead of handing out a result with holes.
template <int KW>
__global__ __launch_bounds__(KMC_U_THREADS)
void kmc_unitig_emit_kernel(KView v, int k, int canon, const uint16_t* __restrict__ adj, const u32* __restrict__ ptr,
                            const u32* __restrict__ dist, const u32* __restrict__ uid_of, const u32* __restrict__ koff_of,
                            const uint8_t* __restrict__ circ, u64 n_unitigs, u64 n_bases, uint8_t* __restrict__ bases,
                            u64* __restrict__ offsets, kmc_ull* __restrict__ abund, uint8_t* __restrict__ flags,
                            kmc_ull* __restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * KMC_U_WAVES + (threadIdx.x >> 6);
    const u64 stride = (u64)gridDim.x * KMC_U_WAVES * 64;
    const int tb = 2 * k - 2;
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[n_unitigs] = n_bases;
    u32 n_circ = 0, n_one = 0, longest = 0;
    u64 total = 0;
    for (u64 base = wave * 64; base < v.n; base += stride) {
        const u64 r = base + lane;
        if (r >= v.n || !(adj[r] >> 10 & 1)) continue;
        const UPlace p = u_place(r, ptr, dist, canon != 0);
        const u64 uid = uid_of[p.first];
        const u64 at = (u64)koff_of[p.first] + uid * (u64)(k - 1);
        const u64 xc = v.cnt[r];
        u64 xlo = v.lo[r], xhi = KW == 2 ? v.hi[r] : 0ull;
        if (uid >= n_unitigs || at + (u64)(k - 1) + p.pos >= n_bases) { atomicAdd(&summary[0], 1ull); continue; }   // (never)
        total += xc;
        atomicAdd(&abund[uid], (kmc_ull)xc);
        if (p.pos != 0) {   // the last character of its reading: the last of x, or the complement of its first
            const u32 top = (u32)((KW == 2 && tb >= 64 ? xhi >> (tb - 64) : xlo >> tb) & 3ull);
            bases[at + (u64)(k - 1) + p.pos] = u_ascii(p.rc ? 3u - top : (u32)(xlo & 3ull));
            continue;
        }
        if (p.rc) { u64 rhi, rlo; revcomp_key(xhi, xlo, k, rhi, rlo); xhi = rhi; xlo = rlo; }
        for (int j = 0; j < k; ++j) {
            const int bit = tb - 2 * j;
            bases[at + j] = u_ascii((u32)((KW == 2 && bit >= 64 ? xhi >> (bit - 64) : xlo >> bit) & 3ull));
        }
        const u32 cf = circ[r] & 1u;
        offsets[uid] = at;
        flags[uid] = (uint8_t)cf;
        n_circ += cf;
        n_one += p.len == 1u ? 1u : 0u;
        longest = p.len > longest ? p.len : longest;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 t = __shfl_xor(longest, o); longest = t > longest ? t : longest; }
    const u64 sc = wave_sum_u64((u64)n_circ), so = wave_sum_u64((u64)n_one), st = wave_sum_u64(total);
    if (lane == 0) {
        if (sc) atomicAdd(&summary[3], (kmc_ull)sc);
        if (so) atomicAdd(&summary[4], (kmc_ull)so);
        if (longest) atomicMax(&summary[5], (kmc_ull)longest);
        if (st) atomicAdd(&summary[7], (kmc_ull)st);
    }
}
