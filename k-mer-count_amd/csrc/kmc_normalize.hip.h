// kmc_normalize.hip.h -- read depth normalised (include/kmc.h: kmc_normalize, kmc_normalize_device): per read a percentile
// of the counts of its windows, a verdict per read (or pair) by the caller's target and floor, and the surviving reads
// written as a new batch in the layout kmc_add_batch_device takes.
//
//   profile   kmc_profile_kernel as it is (kmc_query.hip.h, through profile_launch), into buffers of the normalise call's
//             own: window_count per window START and the five words per read, of which word [0] (V, the valid windows) is
//             read here.  The kernel writes EVERY one of a read's W = L - k + 1 window positions (n_chunks covers k - 1
//             positions past the batch, the store is guarded by the batch's size only) and writes 0 for an invalid window
//             as for an absent key.  So validity is not in window_count, and need not be: the I = W - V invalid windows are
//             I of the smallest entries, and the q-th smallest VALID count is the (q + I)-th smallest of all W entries.
//   select    the hot path: the rank-th smallest of W u32 words per read, by radix selection.  Two variants by W:
//               <= KMC_NM_WAVE_MAX   a wave per read.  Lane l holds entries l, l + 64, ... in KMC_NM_SLOTS registers.  Most
//                                    significant bit first, from the highest bit set in any entry: per bit the lanes count
//                                    their "live and bit clear" entries, ballots over the bits of that count sum it over
//                                    the wave, and the half that holds the rank stays live (n_select_bits).
//               above                a workgroup per read.  Four passes of 8-bit digits over the entries (read from memory
//                                    each pass; they were just written): per-wave 256-bin LDS histograms of the entries that
//                                    match the digits found so far, combined and scanned by the first wave, which finds the
//                                    digit that holds the rank.  Any W below 2^32.
//             The wave kernel walks all reads KMC_NM_TRIP at a time (a lane reads a read's offsets and V and computes its
//             rank), lists the workgroup reads with one atomic per wave and trip, then takes its wave reads one after the other.  The
//             workgroup kernel takes its reads from the list, so the host never waits to learn how many there are.
//   verdict   one lane per read: D (the mate's depth for pairs), the draw, LOW / DEEP / KEEP / EMITTED, read_stats, verdict
//             and the two u32 sequences "emitted" and "emitted length" that kmc_scan.hip.h scans; the summary words are
//             summed per wave and added with one atomic per wave and word.
//   layout    kmc_trim_layout_kernel<true> (whole reads: src = offsets[r]) and kmc_trim_gather_kernel as it is
//   gather    (kmc_trim.hip.h): the control words they read keep their indices.
//
// No kernel waits for another workgroup and every loop is bounded by the batch or by constants.  Every index that comes from
// device data -- an offset, V, a listed read, a rank -- is compared with its array's size before it addresses anything; a
// violation is counted in ctl[KMC_NM_BAD] and the host fails the call.
#pragma once
#include "kmc_trim.hip.h"   // (kmc_trim_layout_kernel, kmc_trim_gather_kernel and their control words)

#define KMC_NM_THREADS 256
#define KMC_NM_WAVES (KMC_NM_THREADS / 64)
#define KMC_NM_SLOTS 16                            // entries a lane holds in the wave variant
#define KMC_NM_TRIP 16                             // reads a wave takes per trip: short trips, many waves in flight
#define KMC_NM_WAVE_MAX (64u * KMC_NM_SLOTS)       // windows: up to here a wave selects in registers, above a workgroup
#define KMC_NM_PSTAT_WORDS 5                       // KMC_PROFILE_WORDS: the row of kmc_profile's read_stats
#define KMC_NM_PAIRED 1u
#define KMC_NM_INVERT 2u
// control words: [0] the total of the scan of "emitted" (u32), [1] of the emitted lengths (u32), [2] valid windows, [3]
// emitted reads, [4] emitted bases, [5] LOW reads, [6] DEEP reads, [7] DEEP reads that are kept, [8] the sum of d_r, [9] range
// violations, [10] reads of 2^32 bases or more, [11] reads listed for the workgroup variant
#define KMC_NM_N_OUT 0
#define KMC_NM_N_BASES 1
#define KMC_NM_VALID 2
#define KMC_NM_EMITTED 3
#define KMC_NM_BASES 4
#define KMC_NM_LOW 5
#define KMC_NM_DEEP 6
#define KMC_NM_DEEP_KEPT 7
#define KMC_NM_DSUM 8
#define KMC_NM_BAD 9
#define KMC_NM_LONG 10
#define KMC_NM_N_GROUP 11
#define KMC_NM_CTL_WORDS 12
static_assert(KMC_NM_N_OUT == KMC_TR_N_OUT && KMC_NM_N_BASES == KMC_TR_N_BASES && KMC_NM_BAD == KMC_TR_BAD,
              "the layout and gather kernels of kmc_trim.hip.h read these control words");
static_assert(KMC_NM_THREADS == KMC_TR_THREADS, "the layout and gather kernels are launched with the trim call's block");

// Read r as the selection sees it: o0 its first base, nw its W window positions, rank the index among ALL W entries sorted
// ascending that holds d_r.  False (and depth 0) if it has no valid window; offsets that do not fit the batch, a V above W
// and a read of 2^32 bases or more are counted.
__device__ __forceinline__ bool n_read(const u64* __restrict__ offsets, const kmc_ull* __restrict__ pstats, u64 n_bases, int k, u32 permille,
                                       u64 r, u64& o0, u32& nw, u32& rank, u64& n_bad, u64& n_long) {
    o0 = offsets[r];
    const u64 o1 = offsets[r + 1];
    if (o0 > o1 || o1 > n_bases) { ++n_bad; return false; }
    const u64 L = o1 - o0;
    if (L >= (1ull << 32)) { ++n_long; return false; }
    const u64 W = L >= (u64)k ? L - (u64)k + 1 : 0;
    const u64 V = pstats[r * KMC_NM_PSTAT_WORDS];
    if (V > W) { ++n_bad; return false; }
    if (!V) return false;
    nw = (u32)W;
    rank = (u32)(((V - 1) * (u64)permille) / 1000ull + (W - V));   // (< W: q <= V - 1)
    return true;
}

// The t-th smallest (from 0) of a wave's live entries: lane l holds v[0 .. NI), bit i of `live` says that v[i] counts; no
// entry has a bit above hb set; t is below the number of live entries.  Most significant bit first: the live entries with
// the bit clear are counted -- per lane a popcount of at most NI, summed over the wave as one ballot per bit of that
// number -- and the half that holds the rank stays live.  No branch inside a bit's step but the choice of the half.
template <int NI>
__device__ __forceinline__ u32 n_select_bits(const u32 (&v)[KMC_NM_SLOTS], u32 live, u32 t, int hb) {
    constexpr int CB = NI == 1 ? 1 : NI == 2 ? 2 : NI == 4 ? 3 : NI == 8 ? 4 : 5;   // bits of a lane's count, 0 .. NI
    u32 prefix = 0;
    for (int b = hb; b >= 0; --b) {
        u32 set = 0, cnt = 0;
#pragma unroll
        for (int i = 0; i < NI; ++i) set |= ((v[i] >> b) & 1u) << i;
        const u32 clear = live & ~set, mine = (u32)__popc(clear);
#pragma unroll
        for (int c = 0; c < CB; ++c) cnt += (u32)__popcll(__builtin_amdgcn_ballot_w64(((mine >> c) & 1u) != 0)) << c;
        if (t < cnt) live = clear;
        else { t -= cnt; live &= set; prefix |= 1u << b; }
    }
    return prefix;
}

// A wave per read of up to KMC_NM_WAVE_MAX windows; the longer ones go onto the list.  depth[r] is written for every read
// the list does not get.
__global__ __launch_bounds__(KMC_NM_THREADS)
void kmc_normalize_select_kernel(const u32* __restrict__ win, const kmc_ull* __restrict__ pstats, const u64* __restrict__ offsets, u64 n_reads,
                                 u64 n_bases, int k, u32 permille, u32* __restrict__ depth, u32* __restrict__ list, kmc_ull* __restrict__ ctl) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u64 n_bad = 0, n_long = 0;
    for (u64 r0 = ((u64)blockIdx.x * KMC_NM_WAVES + wv) * KMC_NM_TRIP; r0 < n_reads; r0 += (u64)gridDim.x * KMC_NM_WAVES * KMC_NM_TRIP) {
        const u64 r = lane < KMC_NM_TRIP ? r0 + lane : n_reads;   // (the other lanes hold no read)
        u64 o0 = 0;
        u32 nw = 0, rank = 0;
        const bool has = r < n_reads && n_read(offsets, pstats, n_bases, k, permille, r, o0, nw, rank, n_bad, n_long);
        const bool group = has && nw > KMC_NM_WAVE_MAX, mine = has && !group;
        if (r < n_reads && !has) depth[r] = 0;
        const u64 mg = __builtin_amdgcn_ballot_w64(group);
        if (mg) {
            u64 base = 0;
            if (lane == 0) base = atomicAdd(&ctl[KMC_NM_N_GROUP], (kmc_ull)__popcll(mg));
            base = __shfl(base, 0);
            const u64 slot = base + (u64)__popcll(mg & ((1ull << lane) - 1ull));
            if (group) {
                if (slot >= n_reads) ++n_bad;
                else list[slot] = (u32)r;   // (the host keeps n_reads below 2^31)
            }
        }
        u64 mm = __builtin_amdgcn_ballot_w64(mine);
        while (mm) {   // (at most KMC_NM_TRIP trips)
            const int src = (int)__builtin_ctzll(mm);
            mm &= mm - 1;
            const u64 so0 = __shfl(o0, src);
            const u32 snw = __shfl(nw, src);
            u32 t = __shfl(rank, src);
            const int ni = (int)((snw + 63u) >> 6);   // slots in use, 1 .. KMC_NM_SLOTS
            u32 v[KMC_NM_SLOTS], live = 0, any = 0;
#pragma unroll
            for (int i = 0; i < KMC_NM_SLOTS; ++i) {
                const u32 j = (u32)lane + 64u * i;
                v[i] = 0;
                if (j < snw) { v[i] = win[so0 + j]; live |= 1u << i; }   // (so0 + j < the read's end <= n_bases)
                any |= v[i];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o);
            // (straight-line code for the next power of two of slots: the slots past ni hold nothing live)
            const int hb = any ? 31 - __builtin_clz(any) : -1;
            const u32 d = ni <= 1 ? n_select_bits<1>(v, live, t, hb) : ni <= 2 ? n_select_bits<2>(v, live, t, hb) : ni <= 4 ? n_select_bits<4>(v, live, t, hb)
                          : ni <= 8 ? n_select_bits<8>(v, live, t, hb) : n_select_bits<KMC_NM_SLOTS>(v, live, t, hb);
            if (lane == 0) depth[r0 + src] = d;
        }
    }
    const u64 sb = wave_sum_u64(n_bad), sl = wave_sum_u64(n_long);
    if (lane == 0) {
        if (sb) atomicAdd(&ctl[KMC_NM_BAD], (kmc_ull)sb);
        if (sl) atomicAdd(&ctl[KMC_NM_LONG], (kmc_ull)sl);
    }
}

// A workgroup per listed read: four passes of 8-bit digits, most significant first.
__global__ __launch_bounds__(KMC_NM_THREADS)
void kmc_normalize_select_group_kernel(const u32* __restrict__ win, const kmc_ull* __restrict__ pstats, const u64* __restrict__ offsets,
                                       u64 n_reads, u64 n_bases, int k, u32 permille, u32* __restrict__ depth, const u32* __restrict__ list,
                                       kmc_ull* __restrict__ ctl) {
    __shared__ u32 hist[KMC_NM_WAVES][256];
    __shared__ u32 found[2];   // the digit that holds the rank, the rank inside it
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    u64 n_listed = ctl[KMC_NM_N_GROUP];
    if (n_listed > n_reads) n_listed = n_reads;
    u64 n_bad = 0;   // thread 0 counts for its workgroup
    for (u64 i = blockIdx.x; i < n_listed; i += gridDim.x) {
        const u64 r = list[i];
        u64 o0 = 0, bad = 0, lng = 0;
        u32 nw = 0, t = 0;
        // (uniform in the workgroup; a listed read has valid windows and offsets that fit)
        if (!(r < n_reads && n_read(offsets, pstats, n_bases, k, permille, r, o0, nw, t, bad, lng))) { ++n_bad; continue; }
        u32 prefix = 0;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const u32 himask = pass ? ~0u << (shift + 8) : 0u;   // the digits found so far
#pragma unroll
            for (int j = 0; j < 4; ++j) hist[wv][lane + 64 * j] = 0;
            __syncthreads();
            for (u64 j = tid; j < nw; j += KMC_NM_THREADS) {
                const u32 x = win[o0 + j];   // (o0 + j < the read's end <= n_bases)
                if (((x ^ prefix) & himask) == 0) atomicAdd(&hist[wv][(x >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wv == 0) {   // lane l: bins 4 l .. 4 l + 3
                u32 c[4], s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    c[j] = 0;
#pragma unroll
                    for (int w = 0; w < KMC_NM_WAVES; ++w) c[j] += hist[w][4 * lane + j];
                    s += c[j];
                }
                u32 incl = s;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const u32 y = __shfl_up(incl, o);
                    if (lane >= o) incl += y;
                }
                u32 below = incl - s;
#pragma unroll
                for (int j = 0; j < 4; ++j) {   // (the live entries number more than t, so exactly one bin holds it)
                    if (t >= below && t - below < c[j]) { found[0] = (u32)(4 * lane + j); found[1] = t - below; }
                    below += c[j];
                }
            }
            __syncthreads();
            prefix |= found[0] << shift;
            t = found[1];
        }
        if (tid == 0) depth[r] = prefix;
    }
    if (tid == 0 && n_bad) atomicAdd(&ctl[KMC_NM_BAD], (kmc_ull)n_bad);
}

struct NormRule {
    u32 permille, flags;
    u64 target, min_depth, seed;
};

// u of unit g at depth D (kmc.h: DRAW)
__device__ __forceinline__ u32 n_draw(u64 seed, u64 g, u32 D) {
    u64 x = seed + (g + 1ull) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (u32)(((x >> 32) * (u64)D) >> 32);
}

// One lane per read (grid stride): read_stats, verdict, emit[r] (0 / 1) and elen[r] (the emitted read's length, else 0)
__global__ __launch_bounds__(KMC_NM_THREADS)
void kmc_normalize_verdict_kernel(NormRule R, const u32* __restrict__ depth, const kmc_ull* __restrict__ pstats, const u64* __restrict__ offsets,
                                  u64 n_reads, uint4* __restrict__ read_stats, uint8_t* __restrict__ verdict, u32* __restrict__ emit,
                                  u32* __restrict__ elen, kmc_ull* __restrict__ ctl) {
    u64 s_valid = 0, s_emit = 0, s_bases = 0, s_low = 0, s_deep = 0, s_kept = 0, s_d = 0, n_bad = 0;
    for (u64 r = (u64)blockIdx.x * KMC_NM_THREADS + threadIdx.x; r < n_reads; r += (u64)gridDim.x * KMC_NM_THREADS) {
        const u64 o0 = offsets[r], o1 = offsets[r + 1];
        u64 L = o1 >= o0 ? o1 - o0 : 0;   // (the select kernel has counted offsets that do not fit and reads too long)
        if (L >= (1ull << 32)) L = 0;
        u64 V = pstats[r * KMC_NM_PSTAT_WORDS];
        if (V > L) V = 0;                 // (counted there as well)
        const u32 d = depth[r];
        u32 D = d;
        u64 g = r;
        if (R.flags & KMC_NM_PAIRED) {
            const u64 m = r ^ 1ull;
            if (m < n_reads) { const u32 dm = depth[m]; D = dm < d ? dm : d; }
            else ++n_bad;   // (the host refuses an odd number of reads)
            g = r >> 1;
        }
        const u32 u = n_draw(R.seed, g, D);
        const bool low = (u64)D < R.min_depth;
        const bool deep = !low && R.target != 0 && (u64)D > R.target;
        const bool keep = !low && (!deep || (u64)u < R.target);
        const bool em = keep != ((R.flags & KMC_NM_INVERT) != 0);
        read_stats[r] = make_uint4((u32)V, d, D, u);
        verdict[r] = (uint8_t)((keep ? 1u : 0u) | (em ? 2u : 0u) | (low ? 4u : 0u) | (deep ? 8u : 0u));
        emit[r] = em ? 1u : 0u;
        elen[r] = em ? (u32)L : 0u;
        s_valid += V; s_emit += em ? 1u : 0u; s_bases += em ? L : 0ull; s_low += low ? 1u : 0u; s_deep += deep ? 1u : 0u;
        s_kept += deep && keep ? 1u : 0u; s_d += d;
    }
    const u64 t0 = wave_sum_u64(s_valid), t1 = wave_sum_u64(s_emit), t2 = wave_sum_u64(s_bases), t3 = wave_sum_u64(s_low);
    const u64 t4 = wave_sum_u64(s_deep), t5 = wave_sum_u64(s_kept), t6 = wave_sum_u64(s_d), t7 = wave_sum_u64(n_bad);
    if ((threadIdx.x & 63) == 0) {
        if (t0) atomicAdd(&ctl[KMC_NM_VALID], (kmc_ull)t0);
        if (t1) atomicAdd(&ctl[KMC_NM_EMITTED], (kmc_ull)t1);
        if (t2) atomicAdd(&ctl[KMC_NM_BASES], (kmc_ull)t2);
        if (t3) atomicAdd(&ctl[KMC_NM_LOW], (kmc_ull)t3);
        if (t4) atomicAdd(&ctl[KMC_NM_DEEP], (kmc_ull)t4);
        if (t5) atomicAdd(&ctl[KMC_NM_DEEP_KEPT], (kmc_ull)t5);
        if (t6) atomicAdd(&ctl[KMC_NM_DSUM], (kmc_ull)t6);
        if (t7) atomicAdd(&ctl[KMC_NM_BAD], (kmc_ull)t7);
    }
}
