// kmc_map.hip.h -- reads threaded through the compacted graph (include/kmc.h: kmc_unitig_map, kmc_unitig_map_device): per
// window of a read the unitig it belongs to, its key position there and its strand; the maximal runs of consecutive
// placements (segments); per-read and per-unitig totals.
//
// What a unitig call leaves on the device is all this needs: adj, the final ranking (ptr / dist) and uid_of.
//   row index   one 8-byte word per view row (kmc_map_index_kernel): low half 2 * unitig + (read on its other strand),
//               high half the key position; a row that is not solid holds KMC_M_NONE in the low half.  A batch has far more
//               windows than the view has rows, so a placement is q_find plus ONE gather instead of adj, ptr / dist, uid_of.
//   place       kmc_profile_kernel's walk over the batch (the chunk front end of kmc_chunks.hip.h: chunks of 1024 positions
//               behind a warm-up chunk, 16 positions per lane) with q_find in the place of the count lookup.
//               The place word goes to the window's START through two LDS transposes (one store instruction = 512
//               contiguous bytes).  The kernel also leaves two bits per position for the passes behind it: "a read starts
//               here" and "the window that ENDS here is valid".
//   segments    a window is a segment HEAD iff it is placed and does not continue its predecessor, a TAIL iff it is placed
//               and its successor does not continue it: both follow from two neighbouring place words and the read-start
//               bit, whatever chunk or wave wrote them.  The i-th head and the i-th tail are the two ends of segment i, and
//               the tail at position j closes segment (heads at positions <= j) - 1, so one scan of the heads per tile
//               (kmc_scan.hip.h) numbers both.  PASS 0 counts heads per tile; PASS 1 scatters the tails' positions, writes
//               seg_offsets at the read starts and adds up the per-read and summary words; PASS 2 writes one 16-byte
//               record per head and one support atomic per segment.  kmc_map_reads_kernel then folds the per-read rows
//               into the three summary words that need complete rows.
//
// No kernel waits for another workgroup and every loop is bounded by the batch, the view or constants.  Every index that
// comes from device data -- a found row, a first-key row, a unitig id, a read index, a scatter position -- is compared
// with its array's size before it addresses anything; a violation is counted in ctl[KMC_M_BAD] and the host fails the call.
#pragma once
#include "kmc_unitig.hip.h"

#define KMC_M_NONE 0xFFFFFFFFu   // KMC_MAP_NONE
#define KMC_M_THREADS 256
#define KMC_M_WAVES (KMC_M_THREADS / 64)
#define KMC_M_TRIPS 8
#define KMC_M_TILE (KMC_M_THREADS * KMC_M_TRIPS)   // positions per compaction tile
#define KMC_M_READ_WORDS 4   // KMC_MAP_READ_WORDS
// control words: [0] the total of the scan (u32), [1] heads counted by PASS 0, [2] valid windows, [3] placed windows,
// [4] crossings, [5] reads with a valid window and all of them placed, [6] reads with no placed window, [7] the most
// segments in one read, [8] range violations, [9] reads of 2^32 bases or more
#define KMC_M_HEADS 1
#define KMC_M_VALID 2
#define KMC_M_PLACED 3
#define KMC_M_CROSS 4
#define KMC_M_FULL 5
#define KMC_M_EMPTY 6
#define KMC_M_MOST 7
#define KMC_M_BAD 8
#define KMC_M_LONG 9
#define KMC_M_CTL_WORDS 10

__device__ __forceinline__ u64 m_word(u32 uni, u32 pos) { return (u64)pos << 32 | uni; }

// idx[r] of every view row; nothing but this kernel writes the index, so the place kernel may trust what it gathers
__global__ __launch_bounds__(KMC_M_THREADS)
void kmc_map_index_kernel(u64 n, const uint16_t* __restrict__ adj, const u32* __restrict__ ptr, const u32* __restrict__ dist,
                          const u32* __restrict__ uid_of, int canon, u64 n_unitigs, u64* __restrict__ idx, kmc_ull* __restrict__ ctl) {
    const u64 r = (u64)blockIdx.x * KMC_M_THREADS + threadIdx.x;
    bool bad = false;
    if (r < n) {
        u64 w = m_word(KMC_M_NONE, 0);
        if (adj[r] >> 10 & 1) {
            const UPlace p = u_place(r, ptr, dist, canon != 0);
            const u32 id = p.first < n ? uid_of[p.first] : KMC_M_NONE;
            if ((u64)id >= n_unitigs || p.pos >= (1u << 31)) bad = true;
            else w = m_word(2u * id + (p.rc ? 1u : 0u), p.pos);
        }
        idx[r] = w;
    }
    const u64 m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[KMC_M_BAD], (kmc_ull)__popcll(m));
}

struct MapLds {
    u32 sbits[KMC_Q_WAVES][64];
    u32 trl[KMC_Q_WAVES][1024], trh[KMC_Q_WAVES][1024];
};

// What the place kernel gathers from: the row index (INDEX), or the arrays it was built from (the A/B behind the index)
struct MapSrc {
    const u64* idx;
    const uint16_t* adj;
    const u32 *ptr, *dist, *uid_of;
    u64 n_unitigs;
};

// place[p] for every p < n_bases, start_bits / valid_bits: one u16 per 16 positions, n_chunks * 64 of each (bit j of word
// p / 16: a read starts at p + j / the window ending at p + j is valid).  The walk over the batch is the chunk front end's (kmc_chunks.hip.h).
template <int KW, bool CANON, bool INDEX>
__global__ __launch_bounds__(KMC_Q_THREADS)
void kmc_map_place_kernel(const uint8_t* __restrict__ bases, u64 n_bases, const u64* __restrict__ offsets, u64 n_reads, int k,
                          u64 n_chunks, u64 chunks_per_wave, QView v, MapSrc src, u64* __restrict__ place,
                          uint16_t* __restrict__ start_bits, uint16_t* __restrict__ valid_bits, kmc_ull* __restrict__ ctl) {
    constexpr int NW = 2 * KW + 1;  // window words: own + 2*KW preceding lanes
    __shared__ MapLds L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 gw = (u64)blockIdx.x * KMC_Q_WAVES + wv;
    const u64 c0 = gw * chunks_per_wave;
    u64 c1 = c0 + chunks_per_wave;
    if (c1 > n_chunks) c1 = n_chunks;
    if (c0 >= c1) return;
    const ChunkKeys<KW> K(k);
    u32 n_bad = 0;

    const u64 cfirst = c0 > 0 ? c0 - 1 : 0;  // warm-up chunk supplies the halo of chunk c0
    ChunkWalk W(offsets, n_reads, cfirst, lane);
    for (u64 c = cfirst; c < c1; ++c) {
        W.step(bases, n_bases, c, true, L.sbits[wv]);
        if (c >= c0) {
            u32 X[NW], Yp[NW + 1];
            const u32 inv16 = chunk_windows<KW>(W, k, X);
            start_bits[c * 64 + lane] = (uint16_t)(W.st & 0xFFFFu);     // (c < n_chunks: inside both arrays)
            valid_bits[c * 64 + lane] = (uint16_t)(~inv16 & 0xFFFFu);
            chunk_rc_stream<KW, CANON>(K, X, Yp);
            u32 uni16[16], pos16[16];
#pragma unroll
            for (int h = 0; h < 16 / KMC_Q_U; ++h) {
                u64 khi[KMC_Q_U], klo[KMC_Q_U];
                u32 row[KMC_Q_U];
                u32 flip = 0, pal = 0;   // bit u: canon took the other strand / the window is its own reverse complement
#pragma unroll
                for (int u = 0; u < KMC_Q_U; ++u) {
                    const ChunkStrand s = chunk_key<KW, CANON>(K, X, Yp, KMC_Q_U * h + u, khi[u], klo[u]);
                    if (s.pal) pal |= 1u << u;
                    if (s.flip) flip |= 1u << u;
                }
                q_find<KW, KMC_Q_U>(v, khi, klo, (~inv16 >> (KMC_Q_U * h)) & ((1u << KMC_Q_U) - 1u), row);
                u64 w[KMC_Q_U];
                if (INDEX) {
#pragma unroll
                    for (int u = 0; u < KMC_Q_U; ++u) {
                        w[u] = m_word(KMC_M_NONE, 0);
                        if (row[u] != KMC_Q_NOPOS) {
                            if ((u64)row[u] < v.n) w[u] = src.idx[row[u]]; else ++n_bad;
                        }
                    }
                } else {
                    // the same word from the arrays the index is built from: three dependent gathers
                    u32 a[KMC_Q_U];
#pragma unroll
                    for (int u = 0; u < KMC_Q_U; ++u) {
                        a[u] = 0;
                        if (row[u] != KMC_Q_NOPOS) {
                            if ((u64)row[u] < v.n) a[u] = src.adj[row[u]]; else ++n_bad;
                        }
                    }
                    UPlace p[KMC_Q_U];
#pragma unroll
                    for (int u = 0; u < KMC_Q_U; ++u)
                        if (a[u] >> 10 & 1) p[u] = u_place(row[u], src.ptr, src.dist, CANON);
#pragma unroll
                    for (int u = 0; u < KMC_Q_U; ++u) {
                        w[u] = m_word(KMC_M_NONE, 0);
                        if (a[u] >> 10 & 1) {
                            const u32 id = (u64)p[u].first < v.n ? src.uid_of[p[u].first] : KMC_M_NONE;
                            if ((u64)id >= src.n_unitigs) ++n_bad;
                            else w[u] = m_word(2u * id + (p[u].rc ? 1u : 0u), p[u].pos);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < KMC_Q_U; ++u) {
                    u32 uni = (u32)w[u];
                    // o: the stored strand, turned if canon turned the window; 0 for a window equal to its reverse complement
                    if (uni != KMC_M_NONE) uni = (pal >> u) & 1 ? uni & ~1u : uni ^ ((flip >> u) & 1u);
                    uni16[KMC_Q_U * h + u] = uni;
                    pos16[KMC_Q_U * h + u] = (u32)(w[u] >> 32);
                }
            }
            {
                u32 *trl = L.trl[wv], *trh = L.trh[wv];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    trl[lane * 16 + ((j + lane) & 15)] = uni16[j];
                    trh[lane * 16 + ((j + lane) & 15)] = pos16[j];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int r = 4 * i + (lane >> 4), col = lane & 15;
                    const u32 xl = trl[r * 16 + ((col + r) & 15)], xh = trh[r * 16 + ((col + r) & 15)];
                    const u64 endp = W.cb + 64u * i + lane;   // the window ends here and starts k - 1 earlier
                    if (endp + 1 >= (u64)k && endp + 1 - (u64)k < n_bases) place[endp + 1 - (u64)k] = m_word(xl, xh);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    }
    const u64 sb = wave_sum_u64((u64)n_bad);
    if (lane == 0 && sb) atomicAdd(&ctl[KMC_M_BAD], (kmc_ull)sb);
}

// window b continues window a (the word-only part of CONTINUES: the caller knows whether b starts a read)
__device__ __forceinline__ bool m_continues(u64 a, u64 b) {
    const u32 ua = (u32)a, ub = (u32)b;
    if (ua == KMC_M_NONE || ua != ub) return false;
    const u32 pa = (u32)(a >> 32), pb = (u32)(b >> 32);
    return (ub & 1u) ? pb + 1u == pa : pb == pa + 1u;
}

// the read that holds position j: the last r in 0..n_reads with offsets[r] <= j (n_reads + 1 if there is none)
__device__ __forceinline__ u64 m_read_of(const u64* __restrict__ offsets, u64 n_reads, u64 j) {
    u64 lo = 0, hi = n_reads + 1;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (offsets[mid] <= j) lo = mid + 1; else hi = mid;
    }
    return lo ? lo - 1 : n_reads + 1;
}

struct MapBatch {
    const u64* place;
    const uint16_t *start_bits, *valid_bits;
    const u64* offsets;
    u64 n_reads, n_bases, n_tiles;
    int k;
};

__device__ __forceinline__ bool m_starts(const MapBatch& b, u64 j) {
    return j == 0 || j >= b.n_bases || (b.start_bits[j >> 4] >> (j & 15) & 1);
}

// The three passes over the positions 0..n_bases (n_bases itself stands for the end: it "starts" the reads whose offset
// it is, and seg_offsets[n_reads]).  A workgroup takes tiles with a grid stride, a tile in KMC_M_TRIPS trips of one
// position per thread.  tile_cnt (PASS 0) / tile_pos (its exclusive scan, PASS 1 and 2) are the compaction scratch.
template <int PASS>
__global__ __launch_bounds__(KMC_M_THREADS)
void kmc_map_segs_kernel(MapBatch b, u32* __restrict__ tile_cnt, const u32* __restrict__ tile_pos, u64 n_segs, u64 n_unitigs,
                         u32* __restrict__ tail_at, uint4* __restrict__ segs, u64* __restrict__ seg_offsets,
                         u32* __restrict__ read_stats, kmc_ull* __restrict__ support, kmc_ull* __restrict__ ctl) {
    __shared__ u32 ws[KMC_M_WAVES];
    __shared__ kmc_ull part[KMC_M_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    u64 n_heads = 0, n_valid = 0, n_placed = 0, n_cross = 0, n_bad = 0;   // this lane's share (lane 0: its wave's, for ballots)
    for (u64 t = blockIdx.x; t < b.n_tiles; t += gridDim.x) {
        u64 run = PASS == 0 ? 0ull : (u64)tile_pos[t];   // heads before this trip's first position
        for (int trip = 0; trip < KMC_M_TRIPS; ++trip) {
            const u64 j = t * KMC_M_TILE + (u64)trip * KMC_M_THREADS + tid;
            const bool in = j < b.n_bases;
            const u64 cur = in ? b.place[j] : m_word(KMC_M_NONE, 0);
            const bool placed = (u32)cur != KMC_M_NONE;
            const bool st = m_starts(b, j);
            bool prev_placed = false, head = false;
            if (placed) {
                const u64 prev = st ? m_word(KMC_M_NONE, 0) : b.place[j - 1];   // (!st: j > 0)
                prev_placed = (u32)prev != KMC_M_NONE;
                head = !m_continues(prev, cur);
            }
            const u64 hm = __builtin_amdgcn_ballot_w64(head);
            if (PASS == 0) {
                if (lane == 0) n_heads += (u64)__popcll(hm);
                continue;
            }
            if (lane == 0) ws[wv] = (u32)__popcll(hm);
            __syncthreads();
            u64 before = run + (u64)__popcll(hm & ((1ull << lane) - 1ull));
            u32 all = 0;
#pragma unroll
            for (int w = 0; w < KMC_M_WAVES; ++w) { if (w < wv) before += ws[w]; all += ws[w]; }
            __syncthreads();
            run += all;
            if (PASS == 1) {
                if (placed) {
                    const bool more = j + 1 < b.n_bases && !m_starts(b, j + 1) && m_continues(cur, b.place[j + 1]);
                    if (!more) {   // a tail: it closes the segment of the last head at or before j
                        const u64 at = before + (head ? 1ull : 0ull) - 1ull;
                        if (at < n_segs) tail_at[at] = (u32)j; else ++n_bad;
                    }
                }
                const bool valid = in && j + (u64)b.k <= b.n_bases &&
                                   (b.valid_bits[(j + (u64)b.k - 1) >> 4] >> ((j + (u64)b.k - 1) & 15) & 1);
                const bool cross = head && !st && prev_placed;
                const u64 vm = __builtin_amdgcn_ballot_w64(valid), pm = __builtin_amdgcn_ballot_w64(placed);
                const u64 cm = __builtin_amdgcn_ballot_w64(cross);
                const u64 sm = __builtin_amdgcn_ballot_w64(st && j <= b.n_bases) | 1ull;
                if (lane == 0) { n_valid += (u64)__popcll(vm); n_placed += (u64)__popcll(pm); n_cross += (u64)__popcll(cm); }
                if (((sm >> lane) & 1) && j <= b.n_bases) {
                    // the run of one read that begins at this lane: up to the next read start of the wave
                    const u64 above = lane == 63 ? 0ull : sm >> (lane + 1);
                    const int len = above ? __ffsll((long long)above) : 64 - lane;
                    const u64 rm = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
                    const u64 rid = m_read_of(b.offsets, b.n_reads, j);
                    if (rid > b.n_reads) ++n_bad;
                    else {
                        if (rid < b.n_reads) {
                            u32* row = read_stats + rid * KMC_M_READ_WORDS;
                            const u32 a0 = (u32)__popcll(vm & rm), a1 = (u32)__popcll(pm & rm), a2 = (u32)__popcll(hm & rm), a3 = (u32)__popcll(cm & rm);
                            if (a0) atomicAdd(&row[0], a0);
                            if (a1) atomicAdd(&row[1], a1);
                            if (a2) atomicAdd(&row[2], a2);
                            if (a3) atomicAdd(&row[3], a3);
                        }
                        if (st)   // every read whose offset is j (empty ones lie before the one that holds j)
                            for (u64 r = rid + 1; r-- > 0 && b.offsets[r] == j;) seg_offsets[r] = before;
                    }
                }
            } else if (head) {
                const u64 rid = m_read_of(b.offsets, b.n_reads, j);
                const u32 uni = (u32)cur;
                if (before >= n_segs || rid >= b.n_reads || (u64)(uni >> 1) >= n_unitigs) { ++n_bad; continue; }
                const u32 len = tail_at[before] - (u32)j + 1u;   // (a segment lies inside a read: fewer than 2^32 windows)
                if (len == 0 || j + len > b.n_bases) { ++n_bad; continue; }
                segs[before] = make_uint4((u32)(j - b.offsets[rid]), len, uni, (u32)(cur >> 32));
                atomicAdd(&support[uni >> 1], (kmc_ull)len);
            }
        }
        if (PASS == 0 && tid == 0) ws[0] = 0;
        if (PASS == 0) {
            // heads of the tile: the waves' counts meet in LDS
            __syncthreads();
            if (lane == 0 && n_heads) atomicAdd(&ws[0], (u32)n_heads);
            __syncthreads();
            if (tid == 0) { tile_cnt[t] = ws[0]; atomicAdd(&ctl[KMC_M_HEADS], (kmc_ull)ws[0]); }
            n_heads = 0;
            __syncthreads();
        }
    }
    // totals: one atomic per workgroup and word
    const u64 sb = wave_sum_u64(n_bad);
    if (lane == 0) { part[wv][0] = sb; part[wv][1] = n_valid; part[wv][2] = n_placed; part[wv][3] = n_cross; }
    __syncthreads();
    if (tid < 4) {
        kmc_ull s = 0;
#pragma unroll
        for (int w = 0; w < KMC_M_WAVES; ++w) s += part[w][tid];
        const int word = tid == 0 ? KMC_M_BAD : tid == 1 ? KMC_M_VALID : tid == 2 ? KMC_M_PLACED : KMC_M_CROSS;
        if (s && (tid == 0 || PASS == 1)) atomicAdd(&ctl[word], s);
    }
}

// Behind PASS 1: the summary words that need a read's complete row, and the reads too long for a u32 window start
__global__ __launch_bounds__(KMC_M_THREADS)
void kmc_map_reads_kernel(const u32* __restrict__ read_stats, const u64* __restrict__ offsets, u64 n_reads, kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull part[KMC_M_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    u64 full = 0, none = 0, lng = 0;
    u32 most = 0;
    for (u64 r = (u64)blockIdx.x * KMC_M_THREADS + tid; r < n_reads; r += (u64)gridDim.x * KMC_M_THREADS) {
        const uint4 s = reinterpret_cast<const uint4*>(read_stats)[r];
        full += s.x && s.y == s.x ? 1u : 0u;
        none += s.y == 0 ? 1u : 0u;
        most = s.z > most ? s.z : most;
        lng += offsets[r + 1] - offsets[r] >= (1ull << 32) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u32 t = __shfl_xor(most, o); most = t > most ? t : most; }
    const u64 sf = wave_sum_u64(full), sn = wave_sum_u64(none), sl = wave_sum_u64(lng);
    if (lane == 0) { part[wv][0] = sf; part[wv][1] = sn; part[wv][2] = most; part[wv][3] = sl; }
    __syncthreads();
    if (tid < 4) {
        kmc_ull s = 0;
#pragma unroll
        for (int w = 0; w < KMC_M_WAVES; ++w) s = tid == 2 ? (part[w][2] > s ? part[w][2] : s) : s + part[w][tid];
        if (s) {
            if (tid == 2) atomicMax(&ctl[KMC_M_MOST], s);
            else atomicAdd(&ctl[tid == 0 ? KMC_M_FULL : tid == 1 ? KMC_M_EMPTY : KMC_M_LONG], s);
        }
    }
}
