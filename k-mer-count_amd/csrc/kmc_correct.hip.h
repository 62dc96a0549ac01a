// kmc_correct.hip.h -- reads corrected against the solid part of the count table (include/kmc.h: kmc_correct,
// kmc_correct_device): substitution errors that leave one clean run of weak windows are replaced by the one base that
// makes every window over them solid.
//
//   mark      kmc_profile_kernel's walk over the batch (the chunk front end of kmc_chunks.hip.h, two lock-step groups of
//             eight q_lookup chains per lane) with the count turned into weak / strong by the range.  It leaves three bits
//             per position for the passes behind it, one u16 per lane and chunk each: "a read starts here", "the window
//             that ENDS here is valid", "... is weak".  Everything behind it works on END positions: the window ending at
//             e starts at e - k + 1, its read neighbours end at e - 1 and e + 1.
//   runs      a run HEAD is a weak window whose predecessor in the read is not weak.  Only runs of at most k windows can
//             be candidates, so a head does not need its tail's position from a pairing pass: it reads the 64 weak bits
//             behind it (k <= 63) and has the length, the two borders, the kind and the suspect position at once -- five
//             u16 loads per head, and heads are rare.  PASS 0 counts the candidates per tile (kmc_scan.hip.h numbers
//             them); PASS 1 writes one record per candidate, cand_offsets at the read starts, and the per-read and
//             summary words (per read: ballots cut at the read starts, as kmc_map_segs_kernel does).
//   try       the hot path: one wave per candidate, lane l < n owns window a + l.  The wave loads the at most 2k - 1 bases
//             the run spans once (two bytes per lane) and turns them into two bit planes with four ballots; a lane cuts
//             its k bits out of each plane and interleaves them into the forward key (planes bit-reversed) and the
//             reverse-complement key (planes complemented) -- no loop over bases.  The two bits of position p are patched
//             in both for the three replacement bases, the smaller key of each pair goes through q_lookup three chains in
//             lock step, and three ballots over "strong or lane >= n" give the accepted mask.  Lane 0 completes the
//             record and, if exactly one base is accepted, writes the one byte into the output copy of the batch.
//             Candidates are independent (kmc.h), so every wave reads the batch as it came.
//
// No kernel waits for another workgroup and every loop is bounded by the batch or by constants.  Every index that comes from
// device data -- a read index, a record slot, a candidate's span -- is compared with its array's size before it addresses
// anything; a violation is counted in ctl[KMC_CR_BAD] and the host fails the call.
#pragma once
#include "kmc_map.hip.h"   // (m_read_of)

#define KMC_CR_THREADS 256
#define KMC_CR_WAVES (KMC_CR_THREADS / 64)
#define KMC_CR_TRIPS 8
#define KMC_CR_TILE (KMC_CR_THREADS * KMC_CR_TRIPS)   // positions per compaction tile
#define KMC_CR_READ_WORDS 4   // KMC_CORRECT_READ_WORDS
// control words: [0] the total of the scan (u32), [1] candidates counted by PASS 0, [2] valid windows, [3] weak windows,
// [4] weak runs, [5] corrected, [6] ambiguous, [7] windows of the corrected candidates, [8] range violations, [9] reads of
// 2^32 bases or more
#define KMC_CR_CANDS 1
#define KMC_CR_VALID 2
#define KMC_CR_WEAK 3
#define KMC_CR_RUNS 4
#define KMC_CR_FIXED 5
#define KMC_CR_AMBIG 6
#define KMC_CR_FIXED_WIN 7
#define KMC_CR_BAD 8
#define KMC_CR_LONG 9
#define KMC_CR_CTL_WORDS 10
#define KMC_CR_INTERIOR 0u
#define KMC_CR_HEAD 1u
#define KMC_CR_TAIL 2u

// start_bits / valid_bits / weak_bits: one u16 per 16 positions, n_chunks * 64 of each (bit j of word p / 16: a read starts
// at p + j / the window ending at p + j is valid / is weak).  The walk over the batch is the chunk front end's.
template <int KW, bool CANON>
__global__ __launch_bounds__(KMC_Q_THREADS)
void kmc_correct_mark_kernel(const uint8_t* __restrict__ bases, u64 n_bases, const u64* __restrict__ offsets, u64 n_reads, int k,
                             u64 n_chunks, u64 chunks_per_wave, QView v, u64 lo_c, u64 hi_c, uint16_t* __restrict__ start_bits,
                             uint16_t* __restrict__ valid_bits, uint16_t* __restrict__ weak_bits) {
    constexpr int NW = 2 * KW + 1;  // window words: own + 2*KW preceding lanes
    __shared__ u32 sbits[KMC_Q_WAVES][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 gw = (u64)blockIdx.x * KMC_Q_WAVES + wv;
    const u64 c0 = gw * chunks_per_wave;
    u64 c1 = c0 + chunks_per_wave;
    if (c1 > n_chunks) c1 = n_chunks;
    if (c0 >= c1) return;
    const ChunkKeys<KW> K(k);
    const u64 cfirst = c0 > 0 ? c0 - 1 : 0;  // warm-up chunk supplies the halo of chunk c0
    ChunkWalk W(offsets, n_reads, cfirst, lane);
    for (u64 c = cfirst; c < c1; ++c) {
        W.step(bases, n_bases, c, true, sbits[wv]);
        if (c >= c0) {
            u32 X[NW], Yp[NW + 1];
            const u32 inv16 = chunk_windows<KW>(W, k, X);
            chunk_rc_stream<KW, CANON>(K, X, Yp);
            u32 weak16 = 0;
#pragma unroll
            for (int h = 0; h < 16 / KMC_Q_U; ++h) {
                u64 khi[KMC_Q_U], klo[KMC_Q_U], out[KMC_Q_U];
#pragma unroll
                for (int u = 0; u < KMC_Q_U; ++u) chunk_key<KW, CANON>(K, X, Yp, KMC_Q_U * h + u, khi[u], klo[u]);
                q_lookup<KW, KMC_Q_U>(v, khi, klo, (~inv16 >> (KMC_Q_U * h)) & ((1u << KMC_Q_U) - 1u), out);
#pragma unroll
                for (int u = 0; u < KMC_Q_U; ++u) weak16 |= (out[u] >= lo_c && out[u] <= hi_c) ? 0u : 1u << (KMC_Q_U * h + u);
            }
            start_bits[c * 64 + lane] = (uint16_t)(W.st & 0xFFFFu);     // (c < n_chunks: inside the three arrays)
            valid_bits[c * 64 + lane] = (uint16_t)(~inv16 & 0xFFFFu);
            weak_bits[c * 64 + lane] = (uint16_t)(weak16 & ~inv16 & 0xFFFFu);
        }
    }
}

struct CorrBatch {
    const uint16_t *start_bits, *valid_bits, *weak_bits;
    const uint8_t* bases;
    const u64* offsets;
    u64 n_reads, n_bases, n_words, n_tiles;   // n_words: u16 words in each bit array
    int k;
};

__device__ __forceinline__ bool c_bit(const uint16_t* __restrict__ a, u64 n_words, u64 j) {
    return (j >> 4) < n_words && (a[j >> 4] >> (j & 15) & 1);
}
// the 64 bits of positions j .. j + 63 (zeros past the array)
__device__ __forceinline__ u64 c_bits64(const uint16_t* __restrict__ a, u64 n_words, u64 j) {
    const u64 w = j >> 4;
    const int s = (int)(j & 15);
    u64 lo = 0, top = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (w + i < n_words) lo |= (u64)a[w + i] << (16 * i);
    if (w + 4 < n_words) top = a[w + 4];
    return s ? (lo >> s) | (top << (64 - s)) : lo;
}
__device__ __forceinline__ bool c_starts(const CorrBatch& b, u64 j) {
    return j == 0 || j >= b.n_bases || c_bit(b.start_bits, b.n_words, j);
}
__device__ __forceinline__ bool c_strong(const CorrBatch& b, u64 e) {
    return c_bit(b.valid_bits, b.n_words, e) && !c_bit(b.weak_bits, b.n_words, e);
}

// the window ending at e is weak: is it the first of its run?  (The window before it in the read ends at e - 1; there is
// none if a read starts where this window starts.)
__device__ __forceinline__ bool c_head(const CorrBatch& b, u64 e) {
    if (e + 1 < (u64)b.k) return false;   // (a valid window cannot end there)
    return e == 0 || c_starts(b, e + 1 - (u64)b.k) || !c_bit(b.weak_bits, b.n_words, e - 1);
}

struct CorrCand { bool is; u32 kind, n; u64 a, p; };   // a: where window a starts, p: the suspect position (both in the batch)

// The run whose first window ends at e, classified: its length up to k, its borders, its kind (kmc.h: CANDIDATE)
__device__ __forceinline__ CorrCand c_classify(const CorrBatch& b, u64 e) {
    CorrCand c = {false, 0, 0, 0, 0};
    const u64 k = (u64)b.k;
    const u64 wk = c_bits64(b.weak_bits, b.n_words, e), st = c_bits64(b.start_bits, b.n_words, e + 2 - k);
    const u64 more = (wk >> 1) & ~st;                 // bit i - 1: the run goes on to the window ending at e + i
    const u32 n = (u32)__ffsll((long long)~more);     // (bit 63 of more is clear)
    if (n > k) return c;
    const u64 be = e + n - 1;                         // the last window ends here
    c.a = e + 1 - k;
    c.n = n;
    const bool l_start = c_starts(b, c.a), l_solid = !l_start && c_strong(b, e - 1);           // (!l_start: a > 0, so e > 0)
    const bool r_end = be + 1 >= b.n_bases || c_bit(b.start_bits, b.n_words, be + 1), r_solid = !r_end && c_strong(b, be + 1);
    if (l_solid && r_solid && n == k) { c.is = true; c.kind = KMC_CR_INTERIOR; c.p = be + 1 - k; }
    else if (l_start && r_solid) { c.is = true; c.kind = KMC_CR_HEAD; c.p = be + 1 - k; }
    else if (l_solid && r_end) { c.is = true; c.kind = KMC_CR_TAIL; c.p = e; }
    return c;
}

// The two passes over the END positions 0..n_bases (n_bases itself stands for the end: it "starts" the reads whose offset it
// is, and cand_offsets[n_reads]).  A workgroup takes tiles with a grid stride, a tile in KMC_CR_TRIPS trips of one position
// per thread.  tile_cnt (PASS 0) / tile_pos (its exclusive scan, PASS 1) are the compaction scratch.  where[2 i], where[2 i
// + 1]: the suspect position of candidate i in the batch and its read, for the try kernel.
template <int PASS>
__global__ __launch_bounds__(KMC_CR_THREADS)
void kmc_correct_runs_kernel(CorrBatch b, u32* __restrict__ tile_cnt, const u32* __restrict__ tile_pos, u64 n_cands,
                             uint4* __restrict__ cands, u64* __restrict__ where, u64* __restrict__ cand_offsets,
                             u32* __restrict__ read_stats, kmc_ull* __restrict__ ctl) {
    __shared__ u32 ws[KMC_CR_WAVES];
    __shared__ kmc_ull part[KMC_CR_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    u64 n_c = 0, n_valid = 0, n_weak = 0, n_runs = 0, n_bad = 0;   // this lane's share (lane 0: its wave's, for ballots)
    for (u64 t = blockIdx.x; t < b.n_tiles; t += gridDim.x) {
        u64 run = PASS == 0 ? 0ull : (u64)tile_pos[t];   // candidates before this trip's first position
        for (int trip = 0; trip < KMC_CR_TRIPS; ++trip) {
            const u64 j = t * KMC_CR_TILE + (u64)trip * KMC_CR_THREADS + tid;
            const bool in = j < b.n_bases;
            const bool weak = in && c_bit(b.weak_bits, b.n_words, j);
            const bool head = weak && c_head(b, j);
            CorrCand cd = {false, 0, 0, 0, 0};
            if (head) cd = c_classify(b, j);
            const u64 cm = __builtin_amdgcn_ballot_w64(cd.is);
            if (PASS == 0) {
                if (lane == 0) n_c += (u64)__popcll(cm);
                continue;
            }
            if (lane == 0) ws[wv] = (u32)__popcll(cm);
            __syncthreads();
            u64 before = run + (u64)__popcll(cm & ((1ull << lane) - 1ull));
            u32 all = 0;
#pragma unroll
            for (int w = 0; w < KMC_CR_WAVES; ++w) { if (w < wv) before += ws[w]; all += ws[w]; }
            __syncthreads();
            run += all;
            const bool st = c_starts(b, j);
            const bool valid = in && c_bit(b.valid_bits, b.n_words, j);
            const u64 vm = __builtin_amdgcn_ballot_w64(valid), wm = __builtin_amdgcn_ballot_w64(weak);
            const u64 hm = __builtin_amdgcn_ballot_w64(head);
            const u64 sm = __builtin_amdgcn_ballot_w64(st && j <= b.n_bases) | 1ull;
            if (lane == 0) { n_valid += (u64)__popcll(vm); n_weak += (u64)__popcll(wm); n_runs += (u64)__popcll(hm); }
            if (((sm >> lane) & 1) && j <= b.n_bases) {
                // the run of one read that begins at this lane: up to the next read start of the wave.  A window belongs to
                // the read that holds its end.
                const u64 above = lane == 63 ? 0ull : sm >> (lane + 1);
                const int len = above ? __ffsll((long long)above) : 64 - lane;
                const u64 rm = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
                const u64 rid = m_read_of(b.offsets, b.n_reads, j);
                if (rid > b.n_reads) ++n_bad;
                else {
                    if (rid < b.n_reads) {
                        u32* row = read_stats + rid * KMC_CR_READ_WORDS;
                        const u32 a0 = (u32)__popcll(vm & rm), a1 = (u32)__popcll(wm & rm), a2 = (u32)__popcll(cm & rm);
                        if (a0) atomicAdd(&row[0], a0);
                        if (a1) atomicAdd(&row[1], a1);
                        if (a2) atomicAdd(&row[2], a2);
                    }
                    if (st)   // every read whose offset is j (empty ones lie before the one that holds j)
                        for (u64 r = rid + 1; r-- > 0 && b.offsets[r] == j;) cand_offsets[r] = before;
                }
            }
            if (cd.is) {
                const u64 rid = m_read_of(b.offsets, b.n_reads, j);
                if (before >= n_cands || rid >= b.n_reads) { ++n_bad; continue; }
                const u64 off = b.offsets[rid];
                if (cd.a < off || cd.p < cd.a || cd.p >= b.n_bases || cd.p - off >= (1ull << 32)) { ++n_bad; continue; }
                const u32 old = b.bases[cd.p];
                cands[before] = make_uint4((u32)(cd.p - off), old | old << 8 | cd.kind << 16, (u32)(cd.a - off), cd.n);
                where[2 * before] = cd.p;
                where[2 * before + 1] = rid;
            }
        }
        if (PASS == 0) {
            // candidates of the tile: the waves' counts meet in LDS
            if (tid == 0) ws[0] = 0;
            __syncthreads();
            if (lane == 0 && n_c) atomicAdd(&ws[0], (u32)n_c);
            __syncthreads();
            if (tid == 0) { tile_cnt[t] = ws[0]; atomicAdd(&ctl[KMC_CR_CANDS], (kmc_ull)ws[0]); }
            n_c = 0;
            __syncthreads();
        }
    }
    if (PASS == 0) return;
    // totals: one atomic per workgroup and word
    const u64 sb = wave_sum_u64(n_bad);
    if (lane == 0) { part[wv][0] = sb; part[wv][1] = n_valid; part[wv][2] = n_weak; part[wv][3] = n_runs; }
    __syncthreads();
    if (tid < 4) {
        kmc_ull s = 0;
#pragma unroll
        for (int w = 0; w < KMC_CR_WAVES; ++w) s += part[w][tid];
        const int word = tid == 0 ? KMC_CR_BAD : tid == 1 ? KMC_CR_VALID : tid == 2 ? KMC_CR_WEAK : KMC_CR_RUNS;
        if (s) atomicAdd(&ctl[word], s);
    }
}

// the reads too long for a u32 position
__global__ __launch_bounds__(KMC_CR_THREADS)
void kmc_correct_reads_kernel(const u64* __restrict__ offsets, u64 n_reads, kmc_ull* __restrict__ ctl) {
    u64 lng = 0;
    for (u64 r = (u64)blockIdx.x * KMC_CR_THREADS + threadIdx.x; r < n_reads; r += (u64)gridDim.x * KMC_CR_THREADS)
        lng += offsets[r + 1] - offsets[r] >= (1ull << 32) ? 1u : 0u;
    const u64 sl = wave_sum_u64(lng);
    if ((threadIdx.x & 63) == 0 && sl) atomicAdd(&ctl[KMC_CR_LONG], (kmc_ull)sl);
}

// bit i of x to bit 2 i
__device__ __forceinline__ u64 c_spread(u32 x) {
    u64 v = x;
    v = (v | v << 16) & 0x0000FFFF0000FFFFull;
    v = (v | v << 8) & 0x00FF00FF00FF00FFull;
    v = (v | v << 4) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | v << 2) & 0x3333333333333333ull;
    v = (v | v << 1) & 0x5555555555555555ull;
    return v;
}
// the key whose 2-bit code i is (bit i of ph, bit i of pl)
__device__ __forceinline__ void c_interleave(u64 ph, u64 pl, u64& hi, u64& lo) {
    lo = c_spread((u32)ph) << 1 | c_spread((u32)pl);
    hi = c_spread((u32)(ph >> 32)) << 1 | c_spread((u32)(pl >> 32));
}
// 2-bit code number i (0..63) of the key replaced
__device__ __forceinline__ void c_patch(u64& hi, u64& lo, int i, u64 code) {
    if (i < 32) lo = (lo & ~(3ull << (2 * i))) | code << (2 * i);
    else hi = (hi & ~(3ull << (2 * i - 64))) | code << (2 * i - 64);
}
__device__ __forceinline__ u32 c_code(u32 byte) {   // (ascii4_to_codes for one byte)
    const u32 t = (byte >> 1) & 3u;
    return t ^ (t >> 1);
}

// One wave per candidate (grid stride): the accepted mask, the record's second word, the corrected byte, the counters.
// bases: the batch as it came; out_bases: its copy, which takes the corrections.
template <int KW, bool CANON>
__global__ __launch_bounds__(KMC_CR_THREADS)
void kmc_correct_try_kernel(const uint8_t* __restrict__ bases, u64 n_bases, u64 n_reads, int k, QView v, u64 lo_c, u64 hi_c,
                            u64 n_cands, uint4* __restrict__ cands, const u64* __restrict__ where, uint8_t* __restrict__ out_bases,
                            u32* __restrict__ read_stats, kmc_ull* __restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    const u64 gw = (u64)blockIdx.x * KMC_CR_WAVES + (threadIdx.x >> 6), n_waves = (u64)gridDim.x * KMC_CR_WAVES;
    const u64 km = (1ull << k) - 1ull;   // (k <= 63)
    u64 n_fixed = 0, n_ambig = 0, n_win = 0, n_bad = 0;   // lane 0 counts for its wave
    for (u64 c = gw; c < n_cands; c += n_waves) {
        const uint4 rec = cands[c];
        const u64 p = where[2 * c], rid = where[2 * c + 1];
        const u32 n = rec.w, back = rec.x - rec.z, kind = (rec.y >> 16) & 255u, old = rec.y & 255u;   // back = p - a
        // lane l < n: window a + l holds p iff l <= back <= l + k - 1; the span a .. a + n + k - 2 lies inside the batch
        if (n == 0 || n > (u32)k || rec.x < rec.z || back + 1 < n || back >= (u32)k || p < back || p - back + n + (u64)k - 1 > n_bases ||
            rid >= n_reads) {
            if (lane == 0) ++n_bad;
            continue;
        }
        const u64 a = p - back;
        const u32 span = n + (u32)k - 1u;   // at most 2 k - 1 <= 125 bases
        u32 b0 = 0, b1 = 0;
        if ((u32)lane < span) b0 = c_code(bases[a + lane]);
        if ((u32)lane + 64u < span) b1 = c_code(bases[a + 64 + lane]);
        const u64 l0 = __builtin_amdgcn_ballot_w64(b0 & 1u), h0 = __builtin_amdgcn_ballot_w64(b0 & 2u);
        const u64 l1 = __builtin_amdgcn_ballot_w64(b1 & 1u), h1 = __builtin_amdgcn_ballot_w64(b1 & 2u);
        // bit i of fl / fh: the low / high bit of base i of this lane's window
        const u64 fl = (lane ? (l0 >> lane) | (l1 << (64 - lane)) : l0) & km, fh = (lane ? (h0 >> lane) | (h1 << (64 - lane)) : h0) & km;
        u64 fhi, flo, rhi = 0, rlo = 0;   // forward: base 0 in the top code; reverse complement: base i complemented in code i
        c_interleave(__builtin_bitreverse64(fh) >> (64 - k), __builtin_bitreverse64(fl) >> (64 - k), fhi, flo);
        if (CANON) c_interleave(~fh & km, ~fl & km, rhi, rlo);
        const bool mine = (u32)lane < n;
        const int ip = mine ? (int)back - lane : 0;   // where p lies in this lane's window
        const u32 oc = c_code(old);
        u64 khi[3], klo[3], out[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const u64 nc = (oc + 1u + (u32)t) & 3u;
            u64 ah = fhi, al = flo;
            c_patch(ah, al, k - 1 - ip, nc);
            if (CANON) {
                u64 bh = rhi, bl = rlo;
                c_patch(bh, bl, ip, 3ull - nc);
                if (key_less(bh, bl, ah, al)) { ah = bh; al = bl; }
            }
            khi[t] = ah; klo[t] = al;
        }
        q_lookup<KW, 3>(v, khi, klo, mine ? 7u : 0u, out);
        u32 mask = 0;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const bool ok = !mine || (out[t] >= lo_c && out[t] <= hi_c);
            if (__builtin_amdgcn_ballot_w64(ok) == ~0ull) mask |= 1u << ((oc + 1u + (u32)t) & 3u);
        }
        if (lane == 0) {
            u32 nb = old;
            if (__popc(mask) == 1) {
                nb = (0x54474341u >> (8 * (__ffs((int)mask) - 1))) & 255u;   // "ACGT"
                out_bases[p] = (uint8_t)nb;
                atomicAdd(&read_stats[rid * KMC_CR_READ_WORDS + 3], 1u);
                ++n_fixed;
                n_win += n;
            } else if (mask) ++n_ambig;
            cands[c].y = old | nb << 8 | kind << 16 | mask << 24;
        }
    }
    if (lane == 0) {
        if (n_fixed) atomicAdd(&ctl[KMC_CR_FIXED], (kmc_ull)n_fixed);
        if (n_ambig) atomicAdd(&ctl[KMC_CR_AMBIG], (kmc_ull)n_ambig);
        if (n_win) atomicAdd(&ctl[KMC_CR_FIXED_WIN], (kmc_ull)n_win);
        if (n_bad) atomicAdd(&ctl[KMC_CR_BAD], (kmc_ull)n_bad);
    }
}
