// kmc_contigs.hip.h -- the counted read walks acted on (include/kmc.h: kmc_unitig_contigs, kmc_unitig_contigs_device): every
// read-resolved repeat gets one copy per matched way through it, links below a support threshold are ignored at the ends
// of single-copy unitigs, and the chains of unitigs that remain are spelled out as contigs with their unitig paths.
//
// What the unitigs, links and transits calls leave on the device is all this needs: u_bases / u_offs / u_abund,
// link_offsets / link_to, link_support / transit_offsets / transit_count.
//   NODES    a lane per unitig recomputes RESOLVED from its at most 16 slots under this call's min_reads (the held verdict
//            byte was made with another call's), writes the copy count (d if resolved, else 1) and sigma in one byte, two
//            bits per row P: the column Q of its one supported slot.  The copy counts are scanned into node_offsets; a lane
//            per unitig then writes its id into node_unitig[] for each of its copies.
//   CHOICE   a lane per node end.  State 2n + 1 is the START end of node n and 2n its END end, so that the join, ranking and
//            cycle kernels of kmc_unitig.hip.h run over the 2 * n_nodes states as they are: their "side L of the smallest
//            row" is the START end of the smallest node.  The lookups are t_records / t_rank of kmc_transits.hip.h.
//   LAYOUT   u_place of kmc_unitig.hip.h per node (always with the smaller-id rule): the start node of its contig, its
//            position, its orientation.  Start nodes are flagged and scanned (contig ids), their node counts are scanned
//            (path_offsets).  Every node writes its path slot, the slot's contig, key count and source position; the key
//            counts are scanned over the slots (G) and slot i of contig c starts at base G[i] + c (k - 1), plus k - 1 if it
//            is not its contig's first.
//   EMIT     a lane per 16 aligned output bytes, as kmc_trim_gather_kernel: the slot of a byte is searched in the slot
//            starts, the 16 bytes at its source position come from two aligned 16-byte loads and a funnel shift, a
//            reversed slot is also byte-reversed (v_perm) and complemented (one xor per byte: 0x15 for A/T, 0x04 for C/G,
//            selected by bit 1 of the byte).  One slot fills most blocks; at most 16 have a byte in one (a slot has one
//            base at least), so the loop is bounded by 16; a piece costs one search of the slot starts and two loads, whatever its length.
//
// No kernel waits for another workgroup and every loop is bounded by the graph or a constant.  Every index that comes from
// device data -- a record index, a target end, a node, a slot, a unitig offset -- is compared with its array's size before
// it addresses anything; a violation is counted in ctl[KMC_CT_BAD] and the host fails the call.
#pragma once
#include "kmc_transits.hip.h"
#include "kmc_trim.hip.h"
#include "kmc_unitig.hip.h"

#define KMC_CT_THREADS 256
#define KMC_CT_WAVES (KMC_CT_THREADS / 64)
// control words (u64): range violations, the nodes as the node kernel adds them up in 64 bits, summary [2] and [3], the
// u32 totals of the four scans (nodes, contigs, path slots, keys), summary [4] .. [6], the keys over the path in 64 bits,
// the join kernel's counter (not used); behind them KMC_U_ROUND_SLOTS u32 counts of the ranking rounds
#define KMC_CT_BAD 0
#define KMC_CT_NODES 1
#define KMC_CT_DUP 2
#define KMC_CT_IGNORED 3
#define KMC_CT_SCAN_N 4
#define KMC_CT_SCAN_C 5
#define KMC_CT_SCAN_P 6
#define KMC_CT_SCAN_G 7
#define KMC_CT_CIRC 8
#define KMC_CT_ONE 9
#define KMC_CT_MOST 10
#define KMC_CT_KEYS 11
#define KMC_CT_UNJOINED 12
#define KMC_CT_CTL_WORDS 13
#define KMC_CT_CTL_BYTES (KMC_CT_CTL_WORDS * sizeof(u64) + KMC_U_ROUND_SLOTS * sizeof(u32))

// copies[u], sigma[u]; ctl: nodes, unitigs duplicated, records ignored for support (at the ends of single-copy unitigs)
__global__ __launch_bounds__(KMC_CT_THREADS)
void kmc_contig_nodes_kernel(TransitGraph g, const u64* __restrict__ transit_offsets, u64 n_slots, const kmc_ull* __restrict__ link_support,
                             const kmc_ull* __restrict__ transit_count, u64 min_reads, u64 min_support, u32* __restrict__ copies,
                             uint8_t* __restrict__ sigma, kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull part[KMC_CT_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 u = (u64)blockIdx.x * KMC_CT_THREADS + tid;
    u32 n = 0, dup = 0, ignored = 0, bad = 0;
    if (u < g.n_unitigs) {
        u64 ls, le;
        u32 ds = 0, de = 0, sg = 0;
        n = 1;
        const u64 t0 = transit_offsets[u], t1 = transit_offsets[u + 1];
        if (!t_records(g, (u32)(2 * u), ls, ds) || !t_records(g, (u32)(2 * u + 1), le, de) || t1 < t0 || t1 - t0 != (u64)ds * de || t1 > n_slots) bad = 1;
        else {
            bool resolved = false;
            if (ds >= 2 && de >= 2) {
                u32 row1 = 0, row2 = 0, col1 = 0, col2 = 0;   // as in kmc_transit_verdict_kernel
#pragma unroll
                for (u32 P = 0; P < 4; ++P)
#pragma unroll
                    for (u32 Q = 0; Q < 4; ++Q)
                        if (P < ds && Q < de && transit_count[t0 + P * de + Q] >= min_reads) {
                            row2 |= row1 & (1u << P); row1 |= 1u << P;
                            col2 |= col1 & (1u << Q); col1 |= 1u << Q;
                            sg |= Q << (2 * P);   // (one Q per row where it matters)
                        }
                resolved = row1 == (1u << ds) - 1u && col1 == (1u << de) - 1u && !row2 && !col2;
            }
            if (resolved) { n = ds; dup = 1; }
            else {
                sg = 0;
                if (min_support)
                    for (u32 i = 0; i < ds + de; ++i) ignored += link_support[i < ds ? ls + i : le + (i - ds)] < min_support ? 1u : 0u;
            }
        }
        copies[u] = n;
        sigma[u] = (uint8_t)sg;
    }
    const u64 s0 = wave_sum_u64((u64)n), s1 = wave_sum_u64((u64)dup), s2 = wave_sum_u64((u64)ignored), s3 = wave_sum_u64((u64)bad);
    if (lane == 0) { part[wv][0] = s0; part[wv][1] = s1; part[wv][2] = s2; part[wv][3] = s3; }
    __syncthreads();
    if (tid < 4) {
        kmc_ull s = 0;
#pragma unroll
        for (int w = 0; w < KMC_CT_WAVES; ++w) s += part[w][tid];
        const int word = tid == 0 ? KMC_CT_NODES : tid == 1 ? KMC_CT_DUP : tid == 2 ? KMC_CT_IGNORED : KMC_CT_BAD;
        if (s) atomicAdd(&ctl[word], s);
    }
}

// node_unitig[node_offsets[u] + p] = u for every copy p of u
__global__ __launch_bounds__(KMC_CT_THREADS)
void kmc_contig_owner_kernel(const u32* __restrict__ copies, const u32* __restrict__ node_offsets, u64 n_unitigs, u64 n_nodes,
                             u32* __restrict__ node_unitig, kmc_ull* __restrict__ ctl) {
    const u64 u = (u64)blockIdx.x * KMC_CT_THREADS + threadIdx.x;
    bool bad = false;
    if (u < n_unitigs) {
        const u32 d = copies[u];
        const u64 at = node_offsets[u];
        if (d < 1 || d > 4 || at + d > n_nodes) bad = true;
        else
            for (u32 p = 0; p < d; ++p) node_unitig[at + p] = (u32)u;
    }
    const u64 m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[KMC_CT_BAD], (kmc_ull)__popcll(m));
}

// the row P of sigma that holds column q, or 4
__device__ __forceinline__ u32 ct_sigma_inv(u32 sg, u32 d, u32 q) {
    u32 r = 4;
#pragma unroll
    for (u32 P = 0; P < 4; ++P)
        if (P < d && r == 4 && ((sg >> (2 * P)) & 3u) == q) r = P;
    return r;
}

// link[a] of node end a: the state of its chosen node end, or KMC_U_NONE
__global__ __launch_bounds__(KMC_CT_THREADS)
void kmc_contig_choice_kernel(TransitGraph g, const kmc_ull* __restrict__ link_support, u64 min_support, const u32* __restrict__ copies,
                              const uint8_t* __restrict__ sigma, const u32* __restrict__ node_offsets, const u32* __restrict__ node_unitig,
                              u64 n_nodes, u32* __restrict__ link, kmc_ull* __restrict__ ctl) {
    const u64 a = (u64)blockIdx.x * KMC_CT_THREADS + threadIdx.x;
    bool bad = false;
    if (a < 2 * n_nodes) {
        u32 out = KMC_U_NONE;
        const u32 n = (u32)(a >> 1), e = (u32)(a & 1) ^ 1u;   // e: 0 START, 1 END
        const u32 u = node_unitig[n];
        u64 lo = 0;
        u32 d = 0;
        if ((u64)u >= g.n_unitigs || node_offsets[u] > n || n - node_offsets[u] >= copies[u] || !t_records(g, 2 * u + e, lo, d)) bad = true;
        else {
            const u32 p = n - node_offsets[u], cu = copies[u], s = 2 * u + e;
            u32 r = 4;   // the rank of the chosen record
            if (cu > 1) {
                r = e == 0 ? p : ((u32)sigma[u] >> (2 * p)) & 3u;
                if (d != cu || r >= d) { bad = true; r = 4; }
            } else {
                u32 live = 0;
#pragma unroll
                for (u32 i = 0; i < 4; ++i)
                    if (i < d && (!min_support || link_support[lo + i] >= min_support)) { ++live; r = i; }
                if (live != 1) r = 4;
            }
            if (r < 4) {
                const u32 t = g.link_to[lo + r], w = t >> 1, f = t & 1u;
                if ((u64)w >= g.n_unitigs) bad = true;
                else {
                    const u32 cw = copies[w];
                    u32 copy = 0;
                    bool have = true;
                    if (cw > 1) {
                        u64 lt;
                        u32 dt;
                        if (!t_records(g, t, lt, dt)) { bad = true; have = false; }
                        else {
                            const u32 q = t_rank(g, lt, dt, s);
                            copy = q == 4 ? 4u : f == 0 ? q : ct_sigma_inv(sigma[w], cw, q);
                            have = copy < cw;   // (no record back, or none of the copies owns it: no choice)
                        }
                    }
                    if (have) {
                        const u64 nn = (u64)node_offsets[w] + copy;
                        if (nn >= n_nodes) bad = true; else out = (u32)(2 * nn) + (f == 0 ? 1u : 0u);
                    }
                }
            }
        }
        link[a] = out;
    }
    const u64 m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[KMC_CT_BAD], (kmc_ull)__popcll(m));
}

// per node: is it the start node of its contig, and if so of how many nodes (0 otherwise): the inputs of two scans
__global__ __launch_bounds__(KMC_CT_THREADS)
void kmc_contig_place_kernel(u64 n_nodes, const u32* __restrict__ ptr, const u32* __restrict__ dist, u32* __restrict__ is_first,
                             u32* __restrict__ first_len) {
    const u64 n = (u64)blockIdx.x * KMC_CT_THREADS + threadIdx.x;
    if (n >= n_nodes) return;
    const UPlace p = u_place(n, ptr, dist, true);
    is_first[n] = p.pos == 0 ? 1u : 0u;
    first_len[n] = p.pos == 0 ? p.len : 0u;
}

struct ContigSrc {
    const u64* u_offs;       // n_unitigs + 1
    const kmc_ull* u_abund;  // n_unitigs
    u64 n_unitigs, u_bases;  // (u_bases: the bases of all unitigs)
};

// dst[at] += val for every lane with at != KMC_T_NONE, equal `at` of the wave combined before the atomic: t_add's leader
// loop (kmc_transits.hip.h) with a sum of values where that one counts lanes.  Every lane of the wave calls it.
__device__ __forceinline__ void ct_add(kmc_ull* __restrict__ dst, u64 at, u64 val, int lane) {
    bool mine = at != KMC_T_NONE;
    kmc_ull left = __builtin_amdgcn_ballot_w64(mine);
    for (int it = 0; it < KMC_T_LEADERS && left; ++it) {   // (wave-uniform: left and who come from ballots alone)
        const int leader = __builtin_ctzll(left);
        const u64 al = __shfl(at, leader);
        const bool same = mine && at == al;
        const kmc_ull who = __builtin_amdgcn_ballot_w64(same);
        const u64 sum = wave_sum_u64(same ? val : 0ull);
        if (lane == leader) atomicAdd(dst + al, (kmc_ull)sum);
        if (same) mine = false;
        left &= ~who;
        if (it == 0 && (who & (who - 1)) == 0) break;
    }
    if (mine) atomicAdd(dst + at, (kmc_ull)val);
}

// Every node writes its path slot: the entry 2u + o, the slot's contig, key count and the unitig base its first output base
// comes from (a reversed slot goes down from there).  Start nodes write path_offsets / flags and feed summary [4] .. [6].
// abund is zero before the launch; the nodes of a wave that lie in one contig add their abundances with one atomic (ct_add).
__global__ __launch_bounds__(KMC_CT_THREADS)
void kmc_contig_path_kernel(u64 n_nodes, u64 n_contigs, int k, const u32* __restrict__ ptr, const u32* __restrict__ dist,
                            const u32* __restrict__ cid_of, const u32* __restrict__ poff_of, const uint8_t* __restrict__ circ,
                            const u32* __restrict__ node_unitig, ContigSrc S, u32* __restrict__ path, u32* __restrict__ slot_cid,
                            u32* __restrict__ slot_keys, u64* __restrict__ slot_src, u64* __restrict__ path_offsets,
                            kmc_ull* __restrict__ abund, uint8_t* __restrict__ flags, kmc_ull* __restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    const u64 n = (u64)blockIdx.x * KMC_CT_THREADS + threadIdx.x;
    u32 n_circ = 0, n_one = 0, most = 0, bad = 0;
    u64 keys = 0, add_at = KMC_T_NONE, add_val = 0;
    if (n == 0) path_offsets[n_contigs] = n_nodes;
    if (n < n_nodes) {
        const UPlace p = u_place(n, ptr, dist, true);
        const u32 u = node_unitig[n];
        if ((u64)p.first >= n_nodes || (u64)u >= S.n_unitigs) bad = 1;
        else {
            const u64 cid = cid_of[p.first], slot = (u64)poff_of[p.first] + p.pos;
            const u64 uo = S.u_offs[u], ue = S.u_offs[u + 1];
            if (cid >= n_contigs || slot >= n_nodes || ue < uo + (u64)k || ue > S.u_bases || ue - uo >= (1ull << 32)) bad = 1;
            else {
                const u64 len = ue - uo, skip = p.pos ? (u64)(k - 1) : 0ull;
                path[slot] = 2 * u + (p.rc ? 1u : 0u);
                slot_cid[slot] = (u32)cid;
                slot_keys[slot] = (u32)(len - (u64)(k - 1));
                slot_src[slot] = p.rc ? uo + len - 1 - skip : uo + skip;
                keys = len - (u64)(k - 1);
                add_at = cid; add_val = S.u_abund[u];
                if (p.pos == 0) {
                    const u32 cf = circ[n] & 1u;
                    path_offsets[cid] = poff_of[p.first];
                    flags[cid] = (uint8_t)cf;
                    n_circ = cf;
                    n_one = p.len == 1u ? 1u : 0u;
                    most = p.len;
                }
            }
        }
    }
    ct_add(abund, add_at, add_val, lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 t = __shfl_xor(most, o); most = t > most ? t : most; }
    const u64 sc = wave_sum_u64((u64)n_circ), so = wave_sum_u64((u64)n_one), sk = wave_sum_u64(keys), sb = wave_sum_u64((u64)bad);
    if (lane == 0) {
        if (sc) atomicAdd(&ctl[KMC_CT_CIRC], (kmc_ull)sc);
        if (so) atomicAdd(&ctl[KMC_CT_ONE], (kmc_ull)so);
        if (most) atomicMax(&ctl[KMC_CT_MOST], (kmc_ull)most);
        if (sk) atomicAdd(&ctl[KMC_CT_KEYS], (kmc_ull)sk);
        if (sb) atomicAdd(&ctl[KMC_CT_BAD], (kmc_ull)sb);
    }
}

// slot_start[i] = G[i] + c (k - 1) (+ k - 1 if slot i is not the first of its contig c); slot_start[n_nodes] = n_bases;
// offsets[c] = the start of its first slot, offsets[n_contigs] = n_bases
__global__ __launch_bounds__(KMC_CT_THREADS)
void kmc_contig_starts_kernel(u64 n_nodes, u64 n_contigs, int k, u64 n_bases, const u32* __restrict__ G, const u32* __restrict__ slot_cid,
                              const u64* __restrict__ path_offsets, u64* __restrict__ slot_start, u64* __restrict__ offsets,
                              kmc_ull* __restrict__ ctl) {
    const u64 i = (u64)blockIdx.x * KMC_CT_THREADS + threadIdx.x;
    bool bad = false;
    if (i == 0) { slot_start[n_nodes] = n_bases; offsets[n_contigs] = n_bases; }
    if (i < n_nodes) {
        const u64 c = slot_cid[i];
        if (c >= n_contigs) bad = true;
        else {
            const bool head = path_offsets[c] == i;
            const u64 at = (u64)G[i] + c * (u64)(k - 1) + (head ? 0ull : (u64)(k - 1));
            slot_start[i] = at;
            if (head) offsets[c] = at;
        }
    }
    const u64 m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[KMC_CT_BAD], (kmc_ull)__popcll(m));
}

__device__ __forceinline__ u32 ct_rev4(u32 w) { return __builtin_amdgcn_perm(w, w, 0x00010203u); }   // byte 0 <-> 3, 1 <-> 2
// the complement of eight ASCII bases: A <-> T is ^ 0x15, C <-> G is ^ 0x04, and bit 1 is set in C and G alone
__device__ __forceinline__ u64 ct_comp8(u64 w) {
    const u64 cg = (w >> 1) & 0x0101010101010101ull;
    return w ^ 0x1515151515151515ull ^ (cg * 0x11ull);
}

// A lane per 16 aligned output bytes, filled slot by slot (kmc_trim_gather_kernel's loop).  A forward slot reads the 16 bytes
// at its source position; a reversed one reads the m bytes that END there, turns the 16 round and complements them.
// unitigs is readable to the next 16-byte boundary past S.u_bases, out has room to the one past n_bases.
__global__ __launch_bounds__(KMC_CT_THREADS)
void kmc_contig_emit_kernel(const uint8_t* __restrict__ unitigs, u64 u_bases, u64 n_nodes, u64 n_bases, const u64* __restrict__ slot_start,
                            const u64* __restrict__ slot_src, const u32* __restrict__ path, uint8_t* __restrict__ out,
                            kmc_ull* __restrict__ ctl) {
    const u64 p = ((u64)blockIdx.x * KMC_CT_THREADS + threadIdx.x) * 16;
    bool bad = false;
    if (p < n_bases) {
        u64 lo = 0, hi = 0;
        u32 j = 0;
#pragma unroll 1
        for (int seg = 0; seg < 16 && j < 16 && p + j < n_bases; ++seg) {
            const u64 pos = p + j;
            const u64 i = m_read_of(slot_start, n_nodes, pos);   // pos < n_bases = slot_start[n_nodes]
            if (i >= n_nodes) { bad = true; break; }
            const u64 b0 = slot_start[i], b1 = slot_start[i + 1];
            if (b1 <= pos || b0 > pos) { bad = true; break; }
            const u64 left = b1 - pos, off = pos - b0;
            const u32 m = left < 16 - j ? (u32)left : 16 - j;
            const bool rc = path[i] & 1u;
            const u64 at = slot_src[i];
            u64 s;   // the lowest unitig byte this piece reads
            if (rc) {
                if (at < off + m - 1) { bad = true; break; }
                s = at - off - (m - 1);
            } else s = at + off;
            if (s + m > u_bases) { bad = true; break; }
            const u32 sh = (u32)(s & 15);
            const uint4* q = reinterpret_cast<const uint4*>(unitigs + (s - sh));
            const uint4 a = q[0];
            uint4 b = make_uint4(0, 0, 0, 0);
            if (sh + m > 16) b = q[1];
            u64 x, y;
            t_funnel(a, b, sh, x, y);
            if (rc) {
                // bytes 0 .. m-1 hold the piece in unitig order: all 16 turned round, then the last m of them moved down
                const u64 rx = (u64)ct_rev4((u32)y) << 32 | ct_rev4((u32)(y >> 32)), ry = (u64)ct_rev4((u32)x) << 32 | ct_rev4((u32)(x >> 32));
                const u32 d = 16 - m;
                if (d >= 8) { x = ry >> (8 * (d - 8)); y = 0; }
                else if (d) { x = rx >> (8 * d) | ry << (64 - 8 * d); y = ry >> (8 * d); }
                else { x = rx; y = ry; }
                x = ct_comp8(x); y = ct_comp8(y);
            }
            t_place(x, y, m, j);
            lo |= x; hi |= y;
            j += m;
        }
        if (!bad) *reinterpret_cast<uint4*>(out + p) = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    }
    const u64 m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[KMC_CT_BAD], (kmc_ull)__popcll(m));
}
