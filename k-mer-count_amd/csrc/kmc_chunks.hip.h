// kmc_chunks.hip.h -- the chunk front end: how a wave turns a batch of reads into k-mer windows.  Shared by the four
// kernels that read a batch this way: kmc_stream_kernel, kmc_extract_hist_kernel, kmc_profile_kernel and
// kmc_map_place_kernel.  Device inline code only: no kernel, no LDS and no global state of its own.
//
// Chunk layout.  The batch is the concatenation of all reads as ASCII (1 B/base) plus offsets[n_reads + 1].  It is cut
// into chunks of KMC_CHUNK = 1024 positions; a wave walks a contiguous run of chunks [c0, c1) in order, behind ONE warm-up
// chunk (cfirst = c0 - 1) that only supplies the halo of chunk c0.  Per chunk lane l owns the 16 positions pp = cb + 16 l ..
// pp + 15: one 16-byte load (a coalesced 1 KiB load per wave), packed to one 32-bit word of 2-bit codes in registers
// (wbe, big-endian: base j at bits 31 - 2j .. 30 - 2j).  Bytes at or past n_bases are never loaded and count as bad.
//
// Read starts.  The wave keeps 64 consecutive entries of offsets in registers (lane l: offsets[rbase + l], `consumed` of
// them already used); those that fall into the chunk are scattered into the wave's 64-word LDS bitmap (sbits, owned by
// the kernel) and read back as 16 bits per lane (st).  A chunk with more read starts than the wave holds reloads the next
// 64 entries until one lies past the chunk's end.  r_first / r_end are the indices of the first offset at or after the
// chunk's begin / end.
//
// Halo.  A window of k <= 31 (KW == 1) / k <= 63 (KW == 2) bases ending in the lane's piece reaches back over at most
// 2 KW pieces: X[d] is the word of lane - d, taken with a wave shuffle from this chunk or, for lane < d, from the previous
// one (pw) -- the bases never pass through LDS.  The break bits travel the same way (zb / pzb).
//
// Validity.  A break is a read start or a bad byte (not one of ACGT, past the end of the batch, padding).  The window
// ENDING at a position is invalid iff a break lies in its last k - 1 positions or a bad byte in its first position:
// inv16 = bits of (smear(Z, k - 1) | B << (k - 1)) over the lane's 16 positions, Z = break bits, B = bad bits.
//
// Keys.  Window j of a lane (ending at pp + j) is a static funnel shift (v_alignbit_b32) of X by 30 - 2j bits, masked to
// 2k bits.  The reverse complement comes from the complemented little-endian words the same way: Yp is that stream
// pre-shifted by the k-dependent amount (Pq words, Pr bits), so that window j is again a funnel shift by 2j bits -- no
// per-base rolling dependency on either strand.  Canonical = the smaller of the two.
#pragma once
#include "kmc_device.hip.h"

#define KMC_CHUNK 1024

// wide bit masks for the validity smear: 64 bits cover the 48-base window of KW==1,
// 128 bits the 80-base window of KW==2
template <int KW> struct WMask;
template <> struct WMask<1> {
    u64 v;
    __device__ __forceinline__ static WMask make(u64 lo, u64) { return {lo}; }
    __device__ __forceinline__ WMask shl(int s) const { return {s >= 64 ? 0 : v << s}; }
    __device__ __forceinline__ WMask operator|(WMask o) const { return {v | o.v}; }
    __device__ __forceinline__ u32 bits16_at(int pos) const { return (u32)(v >> pos) & 0xFFFFu; }
};
template <> struct WMask<2> {
    u64 lo, hi;
    __device__ __forceinline__ static WMask make(u64 l, u64 h) { return {l, h}; }
    __device__ __forceinline__ WMask shl(int s) const {
        if (s == 0) return *this;
        if (s >= 128) return {0, 0};
        if (s >= 64) return {0, lo << (s - 64)};
        return {lo << s, (hi << s) | (lo >> (64 - s))};
    }
    __device__ __forceinline__ WMask operator|(WMask o) const { return {lo | o.lo, hi | o.hi}; }
    __device__ __forceinline__ u32 bits16_at(int pos) const {  // pos == 64 here
        return (u32)(hi >> (pos - 64)) & 0xFFFFu;
    }
};

// OR of m << i for i in [0, t)
template <int KW>
__device__ __forceinline__ WMask<KW> smear(WMask<KW> m, int t) {
    if (t <= 0) return WMask<KW>::make(0, 0);
    int cur = 1;
    while (cur * 2 <= t) { m = m | m.shl(cur); cur *= 2; }
    if (cur < t) m = m | m.shl(t - cur);
    return m;
}

// A wave's walk over its chunks: the state carried from chunk to chunk and what step() leaves about the current one.
struct ChunkWalk {
    const u64* offsets;
    u64 n_reads;
    int lane;
    u64 rbase, held;   // this lane holds offsets[rbase + lane] (all ones past the array) ...
    u32 consumed;      // ... and the first `consumed` lanes' entries lie before the current position
    u32 pw, pzb;       // previous chunk's wbe and zb
    // the current chunk
    u64 cb, pp;        // first position of the chunk / of this lane's piece
    u64 r_first, r_end;
    u32 wbe;           // the piece's 16 bases, big-endian 2-bit codes
    u32 st;            // bit j: a read starts at pp + j
    u32 zb;            // low half: break (read start or bad byte) at pp + j; high half: bad byte at pp + j

    // the first read start at or after the warm-up chunk (binary search, wave-uniform)
    __device__ __forceinline__ ChunkWalk(const u64* __restrict__ offsets_, u64 n_reads_, u64 cfirst, int lane_)
        : offsets(offsets_), n_reads(n_reads_), lane(lane_), consumed(0), pw(0), pzb(0), wbe(0), zb(0) {
        const u64 target = cfirst * KMC_CHUNK;
        u64 lo_i = 0, hi_i = n_reads + 1;  // offsets has n_reads + 1 entries
        while (lo_i < hi_i) {
            const u64 mid = (lo_i + hi_i) >> 1;
            if (offsets[mid] < target) lo_i = mid + 1; else hi_i = mid;
        }
        rbase = lo_i;
        held = (rbase + lane <= n_reads) ? offsets[rbase + lane] : ~0ull;
    }

    // Chunk c, called for c = cfirst, cfirst + 1, ... in order.  sbits: the wave's 64 words of LDS.  live == false
    // (wave-uniform): a padding chunk -- nothing is loaded and every position is bad.
    __device__ __forceinline__ void step(const uint8_t* __restrict__ bases, u64 n_bases, u64 c, bool live, u32* sbits) {
        pw = wbe;
        pzb = zb;
        cb = c * KMC_CHUNK;
        pp = cb + 16u * lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (live && pp < n_bases) v = *reinterpret_cast<const uint4*>(bases + pp);
        Enc16 e = encode16(v);
        u32 bad = 0;
        if (__builtin_amdgcn_ballot_w64((e.x0 | e.x1 | e.x2 | e.x3) != 0) != 0) bad = bad16_from(e);
        if (!live) bad = 0xFFFFu;
        else if (pp + 16 > n_bases) {  // bytes past the end of the batch never form windows
            const u32 nvalid = pp < n_bases ? (u32)(n_bases - pp) : 0;
            bad |= (0xFFFFu << nvalid) & 0xFFFFu;
        }
        wbe = le_to_be(e.wle);
        // read starts of this chunk -> per-lane 16-bit mask, through the wave's LDS bitmap
        // (The loop runs on locals.  On the members, which it reaches through `this`, the compiler threads the back edge
        // into a second copy of the loop body, and kmc_extract_hist_kernel<1>, at its register limit, needs one more
        // dword of scratch.)
        u64 rb = rbase, h = held;
        u32 used = consumed;
        r_first = rb + used;
        sbits[lane] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const u64 cend = cb + KMC_CHUNK;
        for (;;) {
            const bool in = (lane >= (int)used) && (h < cend);
            if (in) {
                const u32 rel = (u32)(h - cb);
                atomicOr(&sbits[rel >> 4], 1u << (rel & 15));
            }
            used += (u32)__popcll(__builtin_amdgcn_ballot_w64(in));
            if (used < 64) break;
            rb += 64;   // the wave's 64 entries are used up: the next 64
            used = 0;
            h = (rb + lane <= n_reads) ? offsets[rb + lane] : ~0ull;
        }
        rbase = rb; held = h; consumed = used;
        r_end = rb + used;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        st = __hip_atomic_load(&sbits[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_wave_barrier();
        zb = ((st | bad) & 0xFFFFu) | (bad << 16);
    }
};

// Behind step(), for a chunk whose windows are wanted (c >= c0): the window words X[d] = word of lane - d, and the
// return value inv16, bit j: the window ending at pp + j is invalid.
template <int KW>
__device__ __forceinline__ u32 chunk_windows(const ChunkWalk& w, int k, u32 (&X)[2 * KW + 1]) {
    constexpr int NW = 2 * KW + 1;
    u32 ZB[NW];
    X[0] = w.wbe; ZB[0] = w.zb;
#pragma unroll
    for (int d = 1; d < NW; ++d) {
        const int src = (w.lane - d) & 63;
        const u32 a = __shfl(w.wbe, src), b = __shfl(w.pw, src);
        const u32 za = __shfl(w.zb, src), zbb = __shfl(w.pzb, src);
        X[d] = w.lane >= d ? a : b;
        ZB[d] = w.lane >= d ? za : zbb;
    }
    u64 zl = 0, zh = 0, bl = 0, bh = 0;
#pragma unroll
    for (int d = 0; d < NW; ++d) {
        const int pos = 16 * (NW - 1 - d);
        const u64 z = ZB[d] & 0xFFFFu, b = ZB[d] >> 16;
        if (pos < 64) { zl |= z << pos; bl |= b << pos; } else { zh |= z << (pos - 64); bh |= b << (pos - 64); }
    }
    const WMask<KW> Z = WMask<KW>::make(zl, zh), B = WMask<KW>::make(bl, bh);
    const WMask<KW> inv = smear<KW>(Z, k - 1) | B.shl(k - 1);
    return inv.bits16_at(16 * (NW - 1));
}

// the uniform key constants of k: the 2k-bit mask and the pre-shift of the reverse-complement stream
template <int KW> struct ChunkKeys {
    u64 mask_lo, mask_hi;
    int Pq, Pr;
    __device__ __forceinline__ explicit ChunkKeys(int k) {
        const int kb = 2 * k;
        mask_lo = kb >= 64 ? ~0ull : ((1ull << kb) - 1);
        mask_hi = kb <= 64 ? 0ull : ((1ull << (kb - 64)) - 1);
        const int P = 32 * (2 * KW + 1) - 30 - kb;
        Pq = P >> 5; Pr = P & 31;
    }
};

// forward key of window j
template <int KW>
__device__ __forceinline__ void chunk_fwd_key(const ChunkKeys<KW>& K, const u32 (&X)[2 * KW + 1], int j, u64& hi, u64& lo) {
    u32 f[2 * KW];
#pragma unroll
    for (int m = 0; m < 2 * KW; ++m) f[m] = alignbit(X[m + 1], X[m], 30 - 2 * j);
    lo = ((u64)f[1] << 32 | f[0]) & K.mask_lo;
    hi = 0;
    if constexpr (KW == 2) hi = ((u64)f[3] << 32 | f[2]) & K.mask_hi;
}

// the reverse-complement stream of X from the LSB end (nothing without CANON: chunk_key does not read it then)
template <int KW, bool CANON>
__device__ __forceinline__ void chunk_rc_stream(const ChunkKeys<KW>& K, const u32 (&X)[2 * KW + 1], u32 (&Yp)[2 * KW + 2]) {
    constexpr int NW = 2 * KW + 1;
    if (CANON) {
        u32 Yw[2 * NW + 1];
#pragma unroll
        for (int m = 0; m < NW; ++m) Yw[m] = rc_word_be(X[NW - 1 - m]);
#pragma unroll
        for (int m = NW; m < 2 * NW + 1; ++m) Yw[m] = 0;
#pragma unroll
        for (int m = 0; m < NW; ++m) {
            u32 rr = 0;
#pragma unroll
            for (int q = 0; q < NW; ++q)
                if (q == K.Pq) rr = alignbit(Yw[m + q + 1], Yw[m + q], K.Pr);
            Yp[m] = rr;
        }
        Yp[NW] = 0;
    }
}

// what the canonical choice did to a window: flip = the key is the reverse strand's, pal = both strands read the same
struct ChunkStrand { bool flip, pal; };

// key of window j: the forward key, with CANON the smaller of it and the reverse complement's
template <int KW, bool CANON>
__device__ __forceinline__ ChunkStrand chunk_key(const ChunkKeys<KW>& K, const u32 (&X)[2 * KW + 1], const u32 (&Yp)[2 * KW + 2], int j,
                                                 u64& hi, u64& lo) {
    ChunkStrand s = {false, false};
    chunk_fwd_key<KW>(K, X, j, hi, lo);
    if (CANON) {
        u32 rw[2 * KW];
#pragma unroll
        for (int m = 0; m < 2 * KW; ++m) rw[m] = alignbit(Yp[m + 1], Yp[m], 2 * j);
        const u64 rlo = ((u64)rw[1] << 32 | rw[0]) & K.mask_lo;
        u64 rhi = 0;
        if constexpr (KW == 2) rhi = ((u64)rw[3] << 32 | rw[2]) & K.mask_hi;
        s.pal = key_equal(rhi, rlo, hi, lo);
        s.flip = key_less(rhi, rlo, hi, lo);
        if (s.flip) { lo = rlo; hi = rhi; }
    }
    return s;
}
