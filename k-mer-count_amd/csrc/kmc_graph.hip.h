// kmc_graph.hip.h -- the de Bruijn graph of the sorted view (include/kmc.h: kmc_graph, kmc_graph_device): per key of the
// view a 16-bit word -- which of its four right and four left extensions are solid, whether a side is a unitig end, whether
// the key is solid itself -- and eight summary words over the solid keys.
//
// Write a key as its k-character string x.  canon(f) = min(f, revcomp(f)) in a canonical ctx, f in a forward one.  A key is
// solid iff it is in the view and lo_c <= count <= hi_c.
//   bit c      (0..3)  canon(x[1:] + c) is solid        (right extension by base c)
//   bit 4 + c  (4..7)  canon(c + x[:-1]) is solid       (left extension by base c)
//   bit 8 / 9          side R / L is a unitig end: its degree (popcount of the nibble) is not 1, or the side of the one
//                      neighbour that faces x has a degree other than 1
//   bit 10             x is solid (a key that is not gets 0)
// The neighbours of the facing side are the four siblings of x that share the overlap -- canon(d + x[1:]) for side R,
// canon(x[:-1] + d) for side L, d in ACGT, whichever strand the neighbour was entered on -- so "side R continues" is
// "R degree 1 and exactly one of canon(d + x[1:]) solid".  A key therefore needs 16 independent count lookups and nothing
// else: no position, no second hop, no other lane.  They go through q_lookup of kmc_query.hip.h in two lock-step rounds of
// eight (the eight extensions, then the eight siblings); the sibling that is x itself is not looked up, its count is at hand
// (both of them in a forward ctx, and in a canonical one unless the view holds a key that is not canonical).
//
// Like the query kernels this is latency, not bandwidth: a key reads 16 or 24 bytes of view and writes 2.  A lane takes one
// key per trip; a wave walks the view with a grid stride and keeps its eight summary words in registers, so the whole launch
// issues eight 64-bit atomics per wave, not per 64 keys.
#pragma once
#include "kmc_query.hip.h"

#define KMC_G_THREADS 256
#define KMC_G_WAVES (KMC_G_THREADS / 64)
#define KMC_G_WORDS 8    // KMC_GRAPH_WORDS

// x[1:] + 0 and 0 + x[:-1] of a 2k-bit key (mask = the 2k-bit ones)
template <int KW>
__device__ __forceinline__ void g_shl2(u64 hi, u64 lo, u64 mask_hi, u64 mask_lo, u64& ohi, u64& olo) {
    olo = (lo << 2) & mask_lo;
    ohi = KW == 2 ? (((hi << 2) | (lo >> 62)) & mask_hi) : 0ull;
}
template <int KW>
__device__ __forceinline__ void g_shr2(u64 hi, u64 lo, u64& ohi, u64& olo) {
    olo = (lo >> 2) | (KW == 2 ? hi << 62 : 0ull);
    ohi = KW == 2 ? hi >> 2 : 0ull;
}
// the first character (bits tb, tb + 1; tb = 2k - 2 is even, so the pair never straddles the words): cleared / or-ed in
template <int KW>
__device__ __forceinline__ void g_top_clear(u64& hi, u64& lo, int tb) {
    if (KW == 2 && tb >= 64) hi &= ~(3ull << (tb - 64)); else lo &= ~(3ull << tb);
}
template <int KW>
__device__ __forceinline__ void g_top_or(u64& hi, u64& lo, int tb, u64 c) {
    if (KW == 2 && tb >= 64) hi |= c << (tb - 64); else lo |= c << tb;
}

// One lane, one key of the view per trip.  adj[i] belongs to view row i.  summary: KMC_G_WORDS words, zero before the launch.
template <int KW, bool CANON>
__global__ __launch_bounds__(KMC_G_THREADS)
void kmc_graph_kernel(QView v, u64 lo_c, u64 hi_c, int k, uint16_t* __restrict__ adj, kmc_ull* __restrict__ summary) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * KMC_G_WAVES + (threadIdx.x >> 6);
    const u64 stride = (u64)gridDim.x * KMC_G_WAVES * 64;
    const int tb = 2 * k - 2;
    const u64 mask_hi = v.max_hi, mask_lo = v.max_lo;
    u32 acc[KMC_G_WORDS];
#pragma unroll
    for (int w = 0; w < KMC_G_WORDS; ++w) acc[w] = 0;
    for (u64 base = wave * 64; base < v.n; base += stride) {
        const u64 i = base + lane;
        const bool act = i < v.n;
        u64 xlo = 0, xhi = 0, xc = 0;
        if (act) {
            xlo = v.lo[i];
            if (KW == 2) xhi = v.hi[i];
            xc = v.cnt[i];
        }
        const bool solid = act && xc >= lo_c && xc <= hi_c;
        u64 rhi = 0, rlo = 0;   // the other strand of x
        if (CANON) revcomp_key(xhi, xlo, k, rhi, rlo);
        u64 khi[8], klo[8], out[8];
        // round 1: the eight extensions.  revcomp(x[1:] + c) = comp(c) + revcomp(x)[:-1], revcomp(c + x[:-1]) = revcomp(x)[1:] + comp(c)
        {
            u64 ahi, alo, bhi, blo, cahi = 0, calo = 0, cbhi = 0, cblo = 0;
            g_shl2<KW>(xhi, xlo, mask_hi, mask_lo, ahi, alo);   // x[1:] + A
            g_shr2<KW>(xhi, xlo, bhi, blo);                     // A + x[:-1]
            if (CANON) {
                g_shr2<KW>(rhi, rlo, cahi, calo);
                g_shl2<KW>(rhi, rlo, mask_hi, mask_lo, cbhi, cblo);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                u64 fhi = ahi, flo = alo | (u64)c;
                u64 ghi = bhi, glo = blo;
                g_top_or<KW>(ghi, glo, tb, (u64)c);
                if (CANON) {
                    u64 qhi = cahi, qlo = calo;
                    g_top_or<KW>(qhi, qlo, tb, (u64)(3 - c));
                    if (key_less(qhi, qlo, fhi, flo)) { fhi = qhi; flo = qlo; }
                    const u64 phi = cbhi, plo = cblo | (u64)(3 - c);
                    if (key_less(phi, plo, ghi, glo)) { ghi = phi; glo = plo; }
                }
                khi[c] = fhi; klo[c] = flo;
                khi[4 + c] = ghi; klo[4 + c] = glo;
            }
        }
        q_lookup<KW, 8>(v, khi, klo, solid ? 0xFFu : 0u, out);
        u32 nb = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) nb |= (out[u] >= lo_c && out[u] <= hi_c) ? 1u << u : 0u;
        // round 2: the eight siblings, d + x[1:] and x[:-1] + d.  revcomp(d + x[1:]) = revcomp(x)[:-1] + comp(d),
        // revcomp(x[:-1] + d) = comp(d) + revcomp(x)[1:]
        u32 self = 0;
        {
            u64 ahi = xhi, alo = xlo, bhi = xhi, blo = xlo & ~3ull, cahi = rhi, calo = rlo & ~3ull, cbhi = rhi, cblo = rlo;
            g_top_clear<KW>(ahi, alo, tb);
            if (CANON) g_top_clear<KW>(cbhi, cblo, tb);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                u64 fhi = ahi, flo = alo;
                g_top_or<KW>(fhi, flo, tb, (u64)d);
                u64 ghi = bhi, glo = blo | (u64)d;
                if (CANON) {
                    const u64 qhi = cahi, qlo = calo | (u64)(3 - d);
                    if (key_less(qhi, qlo, fhi, flo)) { fhi = qhi; flo = qlo; }
                    u64 phi = cbhi, plo = cblo;
                    g_top_or<KW>(phi, plo, tb, (u64)(3 - d));
                    if (key_less(phi, plo, ghi, glo)) { ghi = phi; glo = plo; }
                }
                khi[d] = fhi; klo[d] = flo;
                khi[4 + d] = ghi; klo[4 + d] = glo;
                if (fhi == xhi && flo == xlo) self |= 1u << d;
                if (ghi == xhi && glo == xlo) self |= 16u << d;
            }
        }
        q_lookup<KW, 8>(v, khi, klo, solid ? (~self & 0xFFu) : 0u, out);
        u32 sb = self;   // (x is solid wherever these bits are used)
#pragma unroll
        for (int u = 0; u < 8; ++u) sb |= (out[u] >= lo_c && out[u] <= hi_c) ? 1u << u : 0u;
        const u32 dr = __popc(nb & 15u), dl = __popc(nb >> 4);
        const u32 end_r = !(dr == 1 && __popc(sb & 15u) == 1), end_l = !(dl == 1 && __popc(sb >> 4) == 1);
        if (solid) {
            acc[0] += 1; acc[1] += dr; acc[2] += dl;
            acc[3] += (dr == 0 && dl == 0) ? 1u : 0u;
            acc[4] += ((dr == 0) != (dl == 0)) ? 1u : 0u;
            acc[5] += (dr >= 2 || dl >= 2) ? 1u : 0u;
            acc[6] += end_r + end_l;
            acc[7] += end_r & end_l;
        }
        if (act) adj[i] = solid ? (uint16_t)(nb | (end_r << 8) | (end_l << 9) | (1u << 10)) : (uint16_t)0;
    }
#pragma unroll
    for (int w = 0; w < KMC_G_WORDS; ++w) {
        const u64 s = wave_sum_u64((u64)acc[w]);
        if (lane == 0 && s) atomicAdd(&summary[w], (kmc_ull)s);
    }
}
