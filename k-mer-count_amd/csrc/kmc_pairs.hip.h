// kmc_pairs.hip.h -- pair evidence (include/kmc.h: kmc_unitig_pairs, kmc_unitig_pairs_device): which two unitig ends the
// mates 2i / 2i + 1 of a batch connect, across how many bases, and the insert sizes of the pairs that lie on one unitig.
//
// What a unitigs call and a map call leave on the device is all this needs: u_offs (L_u = u_offs[u + 1] - u_offs[u], m_u =
// L_u - k + 1), segs / seg_offsets.
//   ANCHOR  of a read: its longest segment (s, len, 2u + o, pos), of equally long ones the last.  Out end e = 2u + 1 - o,
//           reach = s + (o ? pos + 1 : m_u - pos) + k - 1: the bases from the read's first base to that end of u.
//   CLASS   of pair i: UNPLACED (a mate without anchor), SPAN (u_A != u_B), PROPER / EVERTED (one unitig, opposite
//           orientations, R = reach_A + reach_B > L_u or not; F = R - L_u), SAME_STRAND (one unitig, one orientation).
//   RECORD  the SPAN pairs grouped by (a, b) = (min, max) of their out ends, ascending: count, sum / min / max of R.
// Kernels.  ANCHOR: a lane per read walks its segments, a loop bounded by the read's segment count, and writes one 16-byte
// row (e, u, reach).  CLASS: a lane per pair reads two rows and writes the class, the ends, the value and one sort key
// (a << end_bits) | b, all-ones for a pair that is not SPAN -- the filler the sort drops; equal histogram bins of a wave are
// added by one lane (t_add of kmc_transits.hip.h: inserts pile up around one mean).  The library's MSD sort with run-length
// turns the keys -- under ACCUMULATE together with the held records' keys, their counts as weights -- into the sorted
// distinct keys and their counts.  RECORDS: a lane per new record unpacks its key.  REDUCE: a lane per pair and per held
// record finds its record by binary search and adds (sum, min, max) to it.  Few records each hit by thousands of lanes is the
// common case, so a workgroup combines in an LDS table of KMC_P_SLOTS records (open addressing on the record index,
// KMC_P_PROBES probes) that it flushes once at its end; what finds no slot goes through a per-wave combine (p_combine, the
// leader loop of t_add with a sum, a min and a max).  PLAIN: every lane issues its own atomics (the A/B of DESIGN.md).
//
// No kernel waits for another workgroup and every loop is bounded by the batch, the graph or a constant.  Every index that
// comes from device data -- a read's segments, a unitig id, a position, an end, a record index, a bin -- is compared with its
// array's size before it addresses anything; a violation is counted in ctl[KMC_P_BAD] and the host fails the call.
#pragma once
#include "kmc_transits.hip.h"

#define KMC_P_THREADS 256
#define KMC_P_WAVES (KMC_P_THREADS / 64)
#define KMC_P_SLOTS 512
#define KMC_P_PROBES 4
#define KMC_P_NONE 0xFFFFFFFFu
// control words: [0..4] pairs per class, [5] the sum of F, [6] range violations, [7] the sum of insert_hist, [8] the sum
// of rec_count, [9] pairs and held records whose key is not among the records
#define KMC_P_CLASS 0
#define KMC_P_SUMF 5
#define KMC_P_BAD 6
#define KMC_P_HIST 7
#define KMC_P_RCOUNT 8
#define KMC_P_MISS 9
#define KMC_P_CTL_WORDS 10

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 x = __shfl_xor(v, o); v = x < v ? x : v; }
    return v;
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 x = __shfl_xor(v, o); v = x > v ? x : v; }
    return v;
}

// anchor[r] = (e, u, reach low, reach high) of read r, e == KMC_P_NONE for a read without a segment
__global__ __launch_bounds__(KMC_P_THREADS)
void kmc_pair_anchor_kernel(const u64* __restrict__ seg_offsets, const uint4* __restrict__ segs, u64 n_reads, u64 n_segs,
                            const u64* __restrict__ u_offs, u64 n_unitigs, int k, uint4* __restrict__ anchor, kmc_ull* __restrict__ ctl) {
    const u64 r = (u64)blockIdx.x * KMC_P_THREADS + threadIdx.x;
    bool bad = false;
    if (r < n_reads) {
        uint4 row = make_uint4(KMC_P_NONE, KMC_P_NONE, 0u, 0u);
        const u64 a = seg_offsets[r], b = seg_offsets[r + 1];
        if (a > b || b > n_segs) bad = true;
        else if (a < b) {
            uint4 best = segs[a];
            for (u64 i = a + 1; i < b; ++i) {   // (the longest, of equally long ones the last)
                const uint4 s = segs[i];
                if (s.y >= best.y) best = s;
            }
            const u64 u = best.z >> 1;
            const u32 o = best.z & 1u;
            if (u >= n_unitigs) bad = true;
            else {
                const u64 lo = u_offs[u], hi = u_offs[u + 1];
                if (hi < lo || hi - lo < (u64)k || (u64)best.w >= hi - lo - (u64)(k - 1)) bad = true;
                else {
                    const u64 m = hi - lo - (u64)(k - 1);
                    const u64 reach = (u64)best.x + (o ? (u64)best.w + 1 : m - best.w) + (u64)(k - 1);
                    row = make_uint4((u32)(2 * u + 1 - o), (u32)u, (u32)reach, (u32)(reach >> 32));
                }
            }
        }
        anchor[r] = row;
    }
    const u64 m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[KMC_P_BAD], (kmc_ull)__popcll(m));
}

// A lane per pair: class, ends, value, the sort key and its weight 1; the insert histogram and the totals
__global__ __launch_bounds__(KMC_P_THREADS)
void kmc_pair_class_kernel(const uint4* __restrict__ anchor, u64 n_pairs, const u64* __restrict__ u_offs, u64 n_unitigs, int end_bits,
                           u64 n_bins, uint8_t* __restrict__ pair_class, u32* __restrict__ pair_ends, u64* __restrict__ pair_value,
                           u64* __restrict__ key, u64* __restrict__ weight, kmc_ull* __restrict__ hist, kmc_ull* __restrict__ ctl) {
    __shared__ kmc_ull part[KMC_P_WAVES][7];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 stride = (u64)gridDim.x * KMC_P_THREADS;
    const u64 rounds = (n_pairs + stride - 1) / stride;   // the same for every lane: t_add is called by whole waves
    u64 n_cls[5] = {0, 0, 0, 0, 0}, sum_f = 0, n_bad = 0;
    for (u64 it = 0; it < rounds; ++it) {
        const u64 i = it * stride + (u64)blockIdx.x * KMC_P_THREADS + tid;
        u64 at_bin = KMC_T_NONE;
        if (i < n_pairs) {
            const uint4 A = anchor[2 * i], B = anchor[2 * i + 1];
            u32 cls = KMC_PAIR_UNPLACED;
            const u32 ea = A.x, eb = B.x;   // (a mate with an anchor keeps its end where the other has none)
            u64 val = 0, kw = ~0ull;
            if ((ea != KMC_P_NONE && ((u64)A.y >= n_unitigs || (ea >> 1) != A.y)) || (eb != KMC_P_NONE && ((u64)B.y >= n_unitigs || (eb >> 1) != B.y))) ++n_bad;
            else if (ea != KMC_P_NONE && eb != KMC_P_NONE) {
                const u64 R = (((u64)A.w << 32) | A.z) + (((u64)B.w << 32) | B.z);
                if (A.y != B.y) {
                    const u64 a = ea < eb ? ea : eb, b = ea < eb ? eb : ea;
                    cls = KMC_PAIR_SPAN; val = R; kw = (a << end_bits) | b;
                } else if ((ea ^ eb) & 1u) {
                    const u64 L = u_offs[A.y + 1] - u_offs[A.y];
                    if (R > L) {
                        cls = KMC_PAIR_PROPER; val = R - L; sum_f += val;
                        at_bin = val < n_bins - 1 ? val : n_bins - 1;
                    } else cls = KMC_PAIR_EVERTED;
                } else cls = KMC_PAIR_SAME_STRAND;
            }
#pragma unroll
            for (u32 j = 0; j < 5; ++j) n_cls[j] += cls == j ? 1u : 0u;   // (no indexed register array)
            pair_class[i] = (uint8_t)cls;
            pair_ends[2 * i] = ea; pair_ends[2 * i + 1] = eb;
            pair_value[i] = val;
            key[i] = kw; weight[i] = 1;
        }
        t_add<true>(hist, at_bin, lane);
    }
    u64 s[7];
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = wave_sum_u64(n_cls[j]);
    s[5] = wave_sum_u64(sum_f); s[6] = wave_sum_u64(n_bad);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 7; ++j) part[wv][j] = s[j];
    }
    __syncthreads();
    if (tid < 7) {
        kmc_ull t = 0;
#pragma unroll
        for (int w = 0; w < KMC_P_WAVES; ++w) t += part[w][tid];
        if (t) atomicAdd(&ctl[tid], t);   // (KMC_P_CLASS + 0..4, KMC_P_SUMF, KMC_P_BAD are words 0..6)
    }
}

// A lane per new record: the sorted distinct key unpacked into its ends, its count, and sum / min / max ready to be added to
__global__ __launch_bounds__(KMC_P_THREADS)
void kmc_pair_records_kernel(const u64* __restrict__ run_key, const u64* __restrict__ run_cnt, u64 n_records, int end_bits, u64 n_ends,
                             u64* __restrict__ rec_key, u32* __restrict__ rec_ends, u64* __restrict__ rec_count, u64* __restrict__ rec_sum,
                             u64* __restrict__ rec_min, u64* __restrict__ rec_max, kmc_ull* __restrict__ ctl) {
    const u64 j = (u64)blockIdx.x * KMC_P_THREADS + threadIdx.x;
    u64 cnt = 0, bad = 0;
    if (j < n_records) {
        const u64 kw = run_key[j];
        const u64 a = kw >> end_bits, b = kw & ((1ull << end_bits) - 1);
        cnt = run_cnt[j];
        if (a >= b || b >= n_ends || (j && run_key[j - 1] >= kw)) bad = 1;
        rec_key[j] = kw;
        rec_ends[2 * j] = (u32)a; rec_ends[2 * j + 1] = (u32)b;
        rec_count[j] = cnt; rec_sum[j] = 0; rec_min[j] = ~0ull; rec_max[j] = 0;
    }
    const u64 sc = wave_sum_u64(cnt), sb = wave_sum_u64(bad);
    if ((threadIdx.x & 63) == 0) {
        if (sc) atomicAdd(&ctl[KMC_P_RCOUNT], (kmc_ull)sc);
        if (sb) atomicAdd(&ctl[KMC_P_BAD], (kmc_ull)sb);
    }
}

// (sum, min, max)[at] takes (vs, vn, vx) of every lane with at != KMC_T_NONE, equal `at` of the wave combined before the
// atomics: t_add's leader loop.  Every lane of the wave calls it.
__device__ __forceinline__ void p_combine(kmc_ull* __restrict__ rsum, kmc_ull* __restrict__ rmin, kmc_ull* __restrict__ rmax, u64 at,
                                          u64 vs, u64 vn, u64 vx, int lane) {
    bool mine = at != KMC_T_NONE;
    kmc_ull left = __builtin_amdgcn_ballot_w64(mine);
    for (int it = 0; it < KMC_T_LEADERS && left; ++it) {   // (wave-uniform: left and who come from ballots alone)
        const int leader = __builtin_ctzll(left);
        const u64 al = __shfl(at, leader);
        const bool same = mine && at == al;
        const kmc_ull who = __builtin_amdgcn_ballot_w64(same);
        const u64 s = wave_sum_u64(same ? vs : 0ull), n = wave_min_u64(same ? vn : ~0ull), x = wave_max_u64(same ? vx : 0ull);
        if (lane == leader) { atomicAdd(rsum + al, (kmc_ull)s); atomicMin(rmin + al, (kmc_ull)n); atomicMax(rmax + al, (kmc_ull)x); }
        if (same) mine = false;
        left &= ~who;
        if (it == 0 && (who & (who - 1)) == 0) break;
    }
    if (mine) { atomicAdd(rsum + at, (kmc_ull)vs); atomicMin(rmin + at, (kmc_ull)vn); atomicMax(rmax + at, (kmc_ull)vx); }
}

// Item i < n_pairs: a SPAN pair adds its R; item n_pairs + j: held record j moves its sum / min / max into the new record set
template <bool TABLE>
__global__ __launch_bounds__(KMC_P_THREADS)
void kmc_pair_reduce_kernel(const uint8_t* __restrict__ pair_class, const u32* __restrict__ pair_ends, const u64* __restrict__ pair_value,
                            u64 n_pairs, const u64* __restrict__ old_key, const u64* __restrict__ old_sum, const u64* __restrict__ old_min,
                            const u64* __restrict__ old_max, u64 n_old, int end_bits, const u64* __restrict__ rec_key, u64 n_records,
                            kmc_ull* __restrict__ rec_sum, kmc_ull* __restrict__ rec_min, kmc_ull* __restrict__ rec_max, kmc_ull* __restrict__ ctl) {
    constexpr int SLOTS = TABLE ? KMC_P_SLOTS : 1;   // (the plain form keeps no table: the A/B runs both at their own occupancy)
    __shared__ u32 tag[SLOTS];
    __shared__ kmc_ull lsum[SLOTS], lmin[SLOTS], lmax[SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    if constexpr (TABLE) {
        for (int s = tid; s < KMC_P_SLOTS; s += KMC_P_THREADS) { tag[s] = KMC_P_NONE; lsum[s] = 0; lmin[s] = ~0ull; lmax[s] = 0; }
        __syncthreads();
    }
    const u64 n_items = n_pairs + n_old;
    const u64 stride = (u64)gridDim.x * KMC_P_THREADS;
    const u64 rounds = (n_items + stride - 1) / stride;   // the same for every lane: p_combine is called by whole waves
    u64 n_miss = 0;
    for (u64 it = 0; it < rounds; ++it) {
        const u64 i = it * stride + (u64)blockIdx.x * KMC_P_THREADS + tid;
        bool have = false;
        u64 kw = 0, vs = 0, vn = 0, vx = 0;
        if (i < n_pairs) {
            if (pair_class[i] == KMC_PAIR_SPAN) {
                const u64 ea = pair_ends[2 * i], eb = pair_ends[2 * i + 1];
                kw = ((ea < eb ? ea : eb) << end_bits) | (ea < eb ? eb : ea);
                vs = vn = vx = pair_value[i];
                have = true;
            }
        } else if (i < n_items) {
            const u64 j = i - n_pairs;
            kw = old_key[j]; vs = old_sum[j]; vn = old_min[j]; vx = old_max[j];
            have = true;
        }
        u64 at = KMC_T_NONE;
        if (have) {
            u64 lo = 0, hi = n_records;   // the first record whose key is not below kw
            for (int step = 0; step < 33 && lo < hi; ++step) {
                const u64 mid = lo + ((hi - lo) >> 1);
                if (rec_key[mid] < kw) lo = mid + 1; else hi = mid;
            }
            if (lo < n_records && rec_key[lo] == kw) at = lo; else ++n_miss;
        }
        if constexpr (TABLE) {
            if (at != KMC_T_NONE) {
                u32 s = ((u32)at * 0x9E3779B1u) >> 16;
                for (int p = 0; p < KMC_P_PROBES; ++p, ++s) {
                    s &= KMC_P_SLOTS - 1;
                    const u32 was = atomicCAS(&tag[s], KMC_P_NONE, (u32)at);
                    if (was == KMC_P_NONE || was == (u32)at) {
                        atomicAdd(&lsum[s], (kmc_ull)vs); atomicMin(&lmin[s], (kmc_ull)vn); atomicMax(&lmax[s], (kmc_ull)vx);
                        at = KMC_T_NONE;
                        break;
                    }
                }
            }
            p_combine(rec_sum, rec_min, rec_max, at, vs, vn, vx, lane);   // what found no slot
        } else if (at != KMC_T_NONE) {
            atomicAdd(rec_sum + at, (kmc_ull)vs); atomicMin(rec_min + at, (kmc_ull)vn); atomicMax(rec_max + at, (kmc_ull)vx);
        }
    }
    if constexpr (TABLE) {
        __syncthreads();
        for (int s = tid; s < KMC_P_SLOTS; s += KMC_P_THREADS) {
            const u64 at = tag[s];
            if (at != KMC_P_NONE && at < n_records) {
                atomicAdd(rec_sum + at, lsum[s]); atomicMin(rec_min + at, lmin[s]); atomicMax(rec_max + at, lmax[s]);
            }
        }
    }
    const u64 sm = wave_sum_u64(n_miss);
    if (lane == 0 && sm) atomicAdd(&ctl[KMC_P_MISS], (kmc_ull)sm);
}

// ctl[KMC_P_HIST] = the sum of insert_hist
__global__ __launch_bounds__(KMC_P_THREADS)
void kmc_pair_hist_sum_kernel(const kmc_ull* __restrict__ hist, u64 n_bins, kmc_ull* __restrict__ ctl) {
    const u64 i = (u64)blockIdx.x * KMC_P_THREADS + threadIdx.x;
    const u64 s = wave_sum_u64(i < n_bins ? (u64)hist[i] : 0ull);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&ctl[KMC_P_HIST], (kmc_ull)s);
}
