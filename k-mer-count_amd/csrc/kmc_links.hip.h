// kmc_links.hip.h -- the links between the unitigs of kmc_unitig.hip.h (include/kmc.h: kmc_unitig_links,
// kmc_unitig_links_device): per unitig END the ends its side state reaches across the solid extensions of adj.
//
// What a unitig call leaves on the device is all this needs: adj (one word per view row), the final ranking (ptr / dist:
// a side state a is a terminal iff ptr[a] == a) and uid_of (the unitig id at the row of a unitig's first key).
//   END of a side    a terminal side T of row r belongs to unitig u = uid_of[u_place(r).first]; it is the END end 2u + 1
//                    iff T is the side the reading leaves r through (L if the key is read on its other strand, else R),
//                    otherwise the START end 2u.
//   records          for every set bit c of that side's nibble, ascending: the neighbour key (the shifts and the strand
//                    choice of kmc_unitig_link_kernel, for every set bit instead of the one), its row through the prefix
//                    index (q_find, eight candidates of a row in lock step), the side that faces back.  A facing side that
//                    is a terminal gives the record "target end"; one that is not (around a palindromic key) is dropped
//                    and counted.
// A row with a terminal side is one lane's work.  Every end is exactly one terminal side state, so the per-end counts are
// plain stores; the pass that fills link_to runs behind their exclusive scan.  The resolved targets of the count pass are
// kept in a scratch of eight u32 per view row, so the fill pass repeats no lookup (FILL with SCRATCH); the same kernel
// without the scratch looks everything up again (DESIGN.md has the measurement behind the choice).
//
// No kernel waits for another workgroup and every loop is bounded by the view or by constants.  Every index that comes from
// device data -- a neighbour's row, a first-key row, a unitig id, a fill position -- is compared with its array's size
// before it addresses anything; a violation is counted in ctl[KMC_L_BAD] and the host fails the call.
#pragma once
#include "kmc_unitig.hip.h"

#define KMC_L_THREADS 256
#define KMC_L_WAVES (KMC_L_THREADS / 64)
#define KMC_L_WORDS 8      // KMC_LINK_WORDS
// control words: [0] the total of the scan (u32), [1..7] summary words 1..7, [8] range violations
#define KMC_L_BAD 8
#define KMC_L_CTL_WORDS 9

// What a lane knows about its own row: whether side R / L is a terminal of a solid key, and the ends they are
struct LRow { bool term[2]; u32 uid, exit; };

template <int KW, bool CANON, bool FILL, bool SCRATCH>
__global__ __launch_bounds__(KMC_L_THREADS)
void kmc_links_kernel(QView v, int k, const uint16_t* __restrict__ adj, const u32* __restrict__ ptr, const u32* __restrict__ dist,
                      const u32* __restrict__ uid_of, u64 n_unitigs, u64 n_links, u32* __restrict__ tgt_of,
                      u32* __restrict__ end_cnt, const u32* __restrict__ end_pos, u32* __restrict__ link_to,
                      kmc_ull* __restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * KMC_L_WAVES + (threadIdx.x >> 6);
    const u64 stride = (u64)gridDim.x * KMC_L_WAVES * 64;
    const int tb = 2 * k - 2;
    const u64 mask_hi = v.max_hi, mask_lo = v.max_lo;
    u32 n_rec = 0, n_self = 0, n_drop = 0, n_bad = 0;
    for (u64 base = wave * 64; base < v.n; base += stride) {
        const u64 r = base + lane;
        const bool act = r < v.n;
        const u32 a = act ? (u32)adj[r] : 0u;
        const bool solid = (a >> 10) & 1;
        LRow me;
        me.term[0] = me.term[1] = false;
        me.uid = 0; me.exit = 0;
        if (solid) {
            const uint2 e = reinterpret_cast<const uint2*>(ptr)[r];
            me.term[0] = e.x == (u32)(2 * r);
            me.term[1] = e.y == (u32)(2 * r + 1);
        }
        bool mine = me.term[0] || me.term[1];
        if (mine) {
            const UPlace p = u_place(r, ptr, dist, CANON);
            const u32 id = p.first < v.n ? uid_of[p.first] : KMC_U_NONE;
            if ((u64)id >= n_unitigs) { ++n_bad; mine = false; }
            me.uid = id;
            me.exit = p.rc ? 1u : 0u;
        }
        const u32 want = !mine ? 0u : (me.term[0] ? a & 0x0Fu : 0u) | (me.term[1] ? a & 0xF0u : 0u);
        u32 tgt[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) tgt[u] = KMC_U_NONE;
        if (FILL && SCRATCH) {   // the count pass resolved them
            if (want) {
                const uint4 t0 = reinterpret_cast<const uint4*>(tgt_of)[2 * r], t1 = reinterpret_cast<const uint4*>(tgt_of)[2 * r + 1];
                tgt[0] = t0.x; tgt[1] = t0.y; tgt[2] = t0.z; tgt[3] = t0.w;
                tgt[4] = t1.x; tgt[5] = t1.y; tgt[6] = t1.z; tgt[7] = t1.w;
            }
        } else if (__builtin_amdgcn_ballot_w64(want != 0) != 0) {
            u64 xlo = 0, xhi = 0;
            if (want) {
                xlo = v.lo[r];
                if (KW == 2) xhi = v.hi[r];
            }
            // the eight extensions and the side of each that faces back (kmc_graph_kernel's first round, kmc_unitig_link_kernel's faces)
            u64 khi[8], klo[8];
            u32 face = 0;   // bit u: neighbour u is entered on its side L
            {
                u64 rhi = 0, rlo = 0, ahi, alo, bhi, blo, cahi = 0, calo = 0, cbhi = 0, cblo = 0;
                g_shl2<KW>(xhi, xlo, mask_hi, mask_lo, ahi, alo);   // x[1:] + A: kept -> entered on L
                g_shr2<KW>(xhi, xlo, bhi, blo);                     // A + x[:-1]: kept -> entered on R
                if (CANON) {
                    revcomp_key(xhi, xlo, k, rhi, rlo);
                    g_shr2<KW>(rhi, rlo, cahi, calo);
                    g_shl2<KW>(rhi, rlo, mask_hi, mask_lo, cbhi, cblo);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    u64 fhi = ahi, flo = alo | (u64)c;
                    u64 ghi = bhi, glo = blo;
                    g_top_or<KW>(ghi, glo, tb, (u64)c);
                    u32 fr = 1u, fl = 0u;
                    if (CANON) {
                        u64 qhi = cahi, qlo = calo;
                        g_top_or<KW>(qhi, qlo, tb, (u64)(3 - c));
                        if (key_less(qhi, qlo, fhi, flo)) { fhi = qhi; flo = qlo; fr = 0u; }
                        const u64 phi = cbhi, plo = cblo | (u64)(3 - c);
                        if (key_less(phi, plo, ghi, glo)) { ghi = phi; glo = plo; fl = 1u; }
                    }
                    khi[c] = fhi; klo[c] = flo;
                    khi[4 + c] = ghi; klo[4 + c] = glo;
                    face |= (fr << c) | (fl << (4 + c));
                }
            }
            u32 pos[8];
            q_find<KW, 8>(v, khi, klo, want, pos);
            // the facing side states: terminal or not, then the end each terminal one is
            u32 t[8], pt[8];
            u32 live = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                t[u] = 0; pt[u] = KMC_U_NONE;
                if ((want >> u) & 1) {
                    if ((u64)pos[u] < v.n) {   // (KMC_Q_NOPOS is not: adj says the key is there)
                        t[u] = 2u * pos[u] + ((face >> u) & 1u);
                        pt[u] = ptr[t[u]];
                        live |= 1u << u;
                    } else ++n_bad;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (!((live >> u) & 1)) continue;
                if (pt[u] != t[u]) { ++n_drop; continue; }
                const UPlace p = u_place(t[u] >> 1, ptr, dist, CANON);
                const u32 id = p.first < v.n ? uid_of[p.first] : KMC_U_NONE;
                if ((u64)id >= n_unitigs) { ++n_bad; continue; }
                tgt[u] = 2u * id + (((t[u] & 1u) == (p.rc ? 1u : 0u)) ? 1u : 0u);
            }
            if (!FILL && SCRATCH && want) {
                reinterpret_cast<uint4*>(tgt_of)[2 * r] = make_uint4(tgt[0], tgt[1], tgt[2], tgt[3]);
                reinterpret_cast<uint4*>(tgt_of)[2 * r + 1] = make_uint4(tgt[4], tgt[5], tgt[6], tgt[7]);
            }
        }
        if (!mine) continue;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!me.term[s]) continue;
            const u32 end = 2u * me.uid + (((u32)s == me.exit) ? 1u : 0u);   // (me.uid < n_unitigs)
            if (!FILL) {
                u32 m = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const u32 x = tgt[4 * s + c];
                    if (x == KMC_U_NONE) continue;
                    ++m;
                    n_self += (x >> 1) == me.uid ? 1u : 0u;
                }
                end_cnt[end] = m;
                n_rec += m;
            } else {
                u64 at = end_pos[end];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const u32 x = tgt[4 * s + c];
                    if (x == KMC_U_NONE) continue;
                    if (at < n_links) link_to[at] = x; else ++n_bad;
                    ++at;
                }
            }
        }
    }
    const u64 sb = wave_sum_u64((u64)n_bad);
    if (lane == 0 && sb) atomicAdd(&ctl[KMC_L_BAD], (kmc_ull)sb);
    if (!FILL) {
        const u64 sr = wave_sum_u64((u64)n_rec), ss = wave_sum_u64((u64)n_self), sd = wave_sum_u64((u64)n_drop);
        if (lane == 0) {
            if (sr) atomicAdd(&ctl[1], (kmc_ull)sr);
            if (ss) atomicAdd(&ctl[4], (kmc_ull)ss);
            if (sd) atomicAdd(&ctl[5], (kmc_ull)sd);
        }
    }
}

// Behind the scan of end_cnt into end_pos: link_offsets[i] = end_pos[i] as a u64, link_offsets[2 * n_unitigs] = n_links, and
// the summary words that are per end or per unitig ([2] ends without a record, [3] with two or more, [6] unitigs without a
// record at either end, [7] the most records at one end).  A lane per unitig.
__global__ __launch_bounds__(KMC_L_THREADS)
void kmc_links_offsets_kernel(const u32* __restrict__ end_cnt, const u32* __restrict__ end_pos, u64 n_unitigs, u64 n_links,
                              u64* __restrict__ link_offsets, kmc_ull* __restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    const u64 u = (u64)blockIdx.x * KMC_L_THREADS + threadIdx.x;
    if (u == 0) link_offsets[2 * n_unitigs] = n_links;
    u32 none = 0, multi = 0, lone = 0, most = 0;
    if (u < n_unitigs) {
        const uint2 c = reinterpret_cast<const uint2*>(end_cnt)[u], p = reinterpret_cast<const uint2*>(end_pos)[u];
        link_offsets[2 * u] = p.x;
        link_offsets[2 * u + 1] = p.y;
        none = (c.x == 0 ? 1u : 0u) + (c.y == 0 ? 1u : 0u);
        multi = (c.x >= 2 ? 1u : 0u) + (c.y >= 2 ? 1u : 0u);
        lone = none == 2 ? 1u : 0u;
        most = c.x > c.y ? c.x : c.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 t = __shfl_xor(most, o); most = t > most ? t : most; }
    const u64 sn = wave_sum_u64((u64)none), sm = wave_sum_u64((u64)multi), sl = wave_sum_u64((u64)lone);
    if (lane == 0) {
        if (sn) atomicAdd(&ctl[2], (kmc_ull)sn);
        if (sm) atomicAdd(&ctl[3], (kmc_ull)sm);
        if (sl) atomicAdd(&ctl[6], (kmc_ull)sl);
        if (most) atomicMax(&ctl[7], (kmc_ull)most);
    }
}
