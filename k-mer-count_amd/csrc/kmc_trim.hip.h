// kmc_trim.hip.h -- reads trimmed and filtered by their solid k-mers (include/kmc.h: kmc_trim, kmc_trim_device): per read
// the strong windows counted and their runs found, a span and a verdict by the caller's rule, and the surviving spans
// written as a new batch in the layout kmc_add_batch_device takes.
//
//   mark      kmc_correct_mark_kernel as it is (kmc_correct.hip.h), into bit arrays of the trim call's own: per END
//             position "the window that ends here is valid" and "... is weak".  Read as 64-bit words here: bit j of word w is
//             position 64 w + j.  Window i of a read that starts at o ends at o + k - 1 + i, so a read's windows are the
//             bit range [o + k - 1, o + L) and strong = valid & ~weak over it.
//   reduce    the first half of the hot path: an ordered reduction of that bit range with the run monoid (TrimRun: length,
//             popcounts, first and last set bit, all-ones prefix and suffix, best run with its start).  A 64-bit word
//             becomes an element by bit tricks (t_word: ctz / clz for the ends, a six-step binary search over shifted ANDs
//             for the longest run), elements combine in order (t_join).  Three variants by the read's number of windows:
//               <= KMC_TR_LANE_MAX   a lane per read (at most KMC_TR_LANE_MAX / 64 + 1 words);
//               <= KMC_TR_WAVE_MAX   a wave per read, lane l owns the l-th contiguous slice of the words;
//               above                a workgroup per read, thread t owns the t-th slice, the waves meet in LDS.
//             The lane kernel walks all reads and lists the longer ones (wave reads from the front of `list`, workgroup
//             reads from its back, counted in two control words, one atomic per wave and list); the group kernels take
//             their reads from the list, so no lane walks a long read alone and the host never waits to learn how many
//             there are.
//   verdict   one lane per read: span by mode, PASS, the mate's PASS for pair flags, the emitted bit, read_stats, verdict,
//             and the two u32 sequences "emitted" and "emitted span length" that kmc_scan.hip.h scans; the summary words are
//             summed per wave and added with one atomic per wave and word.
//   layout    one lane per read behind the scans: out_offsets, origin and the batch position of each emitted span.
//   gather    the second half of the hot path: a lane per 16 aligned output bytes.  m_read_of on out_offsets finds the
//             emitted read of its first byte; the 16 bytes at that byte's source position come from two aligned 16-byte
//             loads and a byte funnel shift.  Where the span ends inside the block the same is done for the next span
//             (found by the same search, which skips empty emitted reads) and the pieces are masked and shifted into
//             place -- no byte loads.  Bytes past the last base up to the 16-byte boundary are written as zero.
//
// No kernel waits for another workgroup and every loop is bounded by the batch or by constants.  Every index that comes from
// device data -- an offset, a listed read, a scan position, a span -- is compared with its array's size before it addresses
// anything; a violation is counted in ctl[KMC_TR_BAD] and the host fails the call.
#pragma once
#include "kmc_correct.hip.h"   // (kmc_correct_mark_kernel, m_read_of)

#define KMC_TR_THREADS 256
#define KMC_TR_WAVES (KMC_TR_THREADS / 64)
#define KMC_TR_LANE_MAX 1024u      // windows: up to here a lane reduces the read
#define KMC_TR_WAVE_MAX 32768u     // windows: up to here a wave does, above a workgroup
#define KMC_TR_READ_WORDS 4        // KMC_TRIM_READ_WORDS
#define KMC_TR_MODE_NONE 0
#define KMC_TR_MODE_ENDS 1
#define KMC_TR_MODE_LONGEST 2
#define KMC_TR_INVERT 1u
#define KMC_TR_PAIR_BOTH 2u
#define KMC_TR_PAIR_EITHER 4u
// control words: [0] the total of the scan of "emitted" (u32), [1] of the emitted span lengths (u32), [2] valid windows,
// [3] strong windows, [4] reads whose own PASS is true, [5] emitted reads, [6] emitted bases, [7] emitted reads with a span
// shorter than the read, [8] the emitted reads' bases before trimming, [9] range violations, [10] reads of 2^32 bases or
// more, [11] reads listed for the wave variant, [12] for the workgroup variant
#define KMC_TR_N_OUT 0
#define KMC_TR_N_BASES 1
#define KMC_TR_VALID 2
#define KMC_TR_STRONG 3
#define KMC_TR_PASSED 4
#define KMC_TR_EMITTED 5
#define KMC_TR_BASES 6
#define KMC_TR_CUT 7
#define KMC_TR_BEFORE 8
#define KMC_TR_BAD 9
#define KMC_TR_LONG 10
#define KMC_TR_N_WAVE 11
#define KMC_TR_N_GROUP 12
#define KMC_TR_CTL_WORDS 13

// The run monoid over a range of window bits.  Positions are window indices of the read.  beg: where the range begins (of
// an empty range: anything); val: valid windows; pop: strong windows; first / last: the first and last strong window (pop >
// 0); pre / suf: strong windows at the range's begin / end without a gap; best / bstart: the longest strong run inside the
// range, the one with the smallest start among equals.
struct TrimRun { u32 len, beg, val, pop, first, last, pre, suf, best, bstart; };

__device__ __forceinline__ TrimRun t_none() { return TrimRun{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// n (1..64) window bits beginning at window `beg`: x strong, vx valid, both in the low n bits
__device__ __forceinline__ TrimRun t_word(u64 x, u64 vx, u32 n, u32 beg) {
    TrimRun r = t_none();
    r.len = n; r.beg = beg; r.val = (u32)__popcll(vx);
    if (!x) return r;
    r.pop = (u32)__popcll(x);
    r.first = beg + (u32)__builtin_ctzll(x);
    r.last = beg + 63u - (u32)__builtin_clzll(x);
    const u64 full = n == 64 ? ~0ull : (1ull << n) - 1ull;
    if (x == full) { r.pre = r.suf = r.best = n; r.bstart = beg; return r; }
    r.pre = (u32)__builtin_ctzll(~x);                  // (x != full: ~x has a set bit below n)
    r.suf = (u32)__builtin_clzll(~(x << (64 - n)));    // (the same bit, shifted, lies above the low zeros)
    // p_s: bit i set iff a run of s ones begins at bit i; cur = the same for the length m found so far
    const u64 p1 = x, p2 = p1 & (p1 >> 1), p4 = p2 & (p2 >> 2), p8 = p4 & (p4 >> 4), p16 = p8 & (p8 >> 8), p32 = p16 & (p16 >> 16);
    u64 cur = ~0ull, t;
    u32 m = 0;
    t = cur & p32;          if (t) { cur = t; m = 32; }
    t = cur & (p16 >> m);   if (t) { cur = t; m += 16; }
    t = cur & (p8 >> m);    if (t) { cur = t; m += 8; }
    t = cur & (p4 >> m);    if (t) { cur = t; m += 4; }
    t = cur & (p2 >> m);    if (t) { cur = t; m += 2; }
    t = cur & (p1 >> m);    if (t) { cur = t; m += 1; }
    r.best = m;                                        // (x != 0: m >= 1; x != full: m <= 63)
    r.bstart = beg + (u32)__builtin_ctzll(cur);
    return r;
}

// a then b, b's range right behind a's
__device__ __forceinline__ TrimRun t_join(const TrimRun& a, const TrimRun& b) {
    TrimRun r;
    r.len = a.len + b.len;
    r.beg = a.len ? a.beg : b.beg;
    r.val = a.val + b.val;
    r.pop = a.pop + b.pop;
    r.first = a.pop ? a.first : b.first;
    r.last = b.pop ? b.last : a.last;
    r.pre = a.pre == a.len ? a.len + b.pre : a.pre;
    r.suf = b.suf == b.len ? b.len + a.suf : b.suf;
    // the candidates in the order of their starts: a's best, the run across the seam, b's best; a later one must be longer
    r.best = a.best; r.bstart = a.bstart;
    const u32 mid = a.suf + b.pre;
    if (mid > r.best) { r.best = mid; r.bstart = b.beg - a.suf; }
    if (b.best > r.best) { r.best = b.best; r.bstart = b.bstart; }
    return r;
}

__device__ __forceinline__ TrimRun t_shfl_down(const TrimRun& a, int o) {
    TrimRun r;
    r.len = __shfl_down(a.len, o); r.beg = __shfl_down(a.beg, o); r.val = __shfl_down(a.val, o); r.pop = __shfl_down(a.pop, o);
    r.first = __shfl_down(a.first, o); r.last = __shfl_down(a.last, o); r.pre = __shfl_down(a.pre, o); r.suf = __shfl_down(a.suf, o);
    r.best = __shfl_down(a.best, o); r.bstart = __shfl_down(a.bstart, o);
    return r;
}
// the wave's elements joined in lane order; the result is lane 0's
__device__ __forceinline__ TrimRun t_wave_join(TrimRun a) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const TrimRun b = t_shfl_down(a, o);   // lane l holds lanes l .. l + o - 1, lane l + o the o behind them
        a = t_join(a, b);
    }
    return a;
}

struct TrimBits { const u64 *valid, *weak; u64 n_words; };   // n_words: 64-bit words in each array

// the bit range [a, b) of the batch's END positions, words w0 .. w1 - 1 of it, as one element (window 0 ends at a)
__device__ __forceinline__ TrimRun t_slice(const TrimBits& B, u64 a, u64 b, u64 w0, u64 w1) {
    TrimRun acc = t_none();
    for (u64 w = w0; w < w1; ++w) {
        const u64 p0 = w << 6;
        const u64 s = a > p0 ? a - p0 : 0, t = b < p0 + 64 ? b - p0 : 64;   // (the caller's words meet the range: s < t <= 64)
        if (s >= t) continue;
        u64 vx = 0, wx = 0;
        if (w < B.n_words) { vx = B.valid[w]; wx = B.weak[w]; }
        const u32 n = (u32)(t - s);
        const u64 m = n == 64 ? ~0ull : (1ull << n) - 1ull;
        vx = (vx >> s) & m;
        acc = t_join(acc, t_word(vx & ~(wx >> s), vx, n, (u32)(p0 + s - a)));
    }
    return acc;
}

// runs[2 r], runs[2 r + 1]: (V, S, F, E), (B, N, 0, 0) of read r (kmc.h: STRONG RUN)
__device__ __forceinline__ void t_store(uint4* __restrict__ runs, u64 r, const TrimRun& e) {
    runs[2 * r] = make_uint4(e.val, e.pop, e.first, e.last);
    runs[2 * r + 1] = make_uint4(e.bstart, e.best, 0, 0);
}

// The window bit range of read r: false if its offsets do not fit the batch or it has 2^32 bases or more (counted).
__device__ __forceinline__ bool t_range(const u64* __restrict__ offsets, u64 n_bases, int k, u64 r, u64& a, u64& b, u64& n_bad, u64& n_long) {
    const u64 o0 = offsets[r], o1 = offsets[r + 1];
    if (o0 > o1 || o1 > n_bases) { ++n_bad; return false; }
    if (o1 - o0 >= (1ull << 32)) { ++n_long; return false; }
    a = o0 + (u64)k - 1;
    b = o1;
    if (a > b) a = b;   // (no window)
    return true;
}

// A lane per read; the reads of more than KMC_TR_LANE_MAX windows go onto the list.
__global__ __launch_bounds__(KMC_TR_THREADS)
void kmc_trim_reduce_kernel(TrimBits B, const u64* __restrict__ offsets, u64 n_reads, u64 n_bases, int k, uint4* __restrict__ runs,
                            u32* __restrict__ list, kmc_ull* __restrict__ ctl) {
    const int lane = threadIdx.x & 63;
    u64 n_bad = 0, n_long = 0;
    // a wave takes 64 consecutive reads per trip and stays together: its listed reads share one atomic per list
    for (u64 r0 = (u64)blockIdx.x * KMC_TR_THREADS + (threadIdx.x - lane); r0 < n_reads; r0 += (u64)gridDim.x * KMC_TR_THREADS) {
        const u64 r = r0 + lane;
        u64 a = 0, b = 0;
        const bool ok = r < n_reads && t_range(offsets, n_bases, k, r, a, b, n_bad, n_long);
        const u64 nw = b - a;
        const bool mine = ok && nw <= KMC_TR_LANE_MAX, wave = ok && !mine && nw <= KMC_TR_WAVE_MAX, group = ok && !mine && !wave;
        if (r < n_reads && !ok) t_store(runs, r, t_none());
        if (mine) t_store(runs, r, nw ? t_slice(B, a, b, a >> 6, ((b - 1) >> 6) + 1) : t_none());
        const u64 mw = __builtin_amdgcn_ballot_w64(wave), mg = __builtin_amdgcn_ballot_w64(group);
        if (mw | mg) {
            u64 base_w = 0, base_g = 0;
            if (lane == 0) {
                if (mw) base_w = atomicAdd(&ctl[KMC_TR_N_WAVE], (kmc_ull)__popcll(mw));
                if (mg) base_g = atomicAdd(&ctl[KMC_TR_N_GROUP], (kmc_ull)__popcll(mg));
            }
            base_w = __shfl(base_w, 0); base_g = __shfl(base_g, 0);
            const u64 below = (1ull << lane) - 1ull;
            const u64 slot = wave ? base_w + (u64)__popcll(mw & below) : base_g + (u64)__popcll(mg & below);
            if (wave || group) {
                if (slot >= n_reads) ++n_bad;
                else list[wave ? slot : n_reads - 1 - slot] = (u32)r;   // (the host keeps n_reads below 2^32)
            }
        }
    }
    const u64 sb = wave_sum_u64(n_bad), sl = wave_sum_u64(n_long);
    if ((threadIdx.x & 63) == 0) {
        if (sb) atomicAdd(&ctl[KMC_TR_BAD], (kmc_ull)sb);
        if (sl) atomicAdd(&ctl[KMC_TR_LONG], (kmc_ull)sl);
    }
}

// G == 64: a wave per listed read; G == KMC_TR_THREADS: a workgroup per listed read.  Member g of the group owns the g-th
// slice of ceil(words / G) words.
template <int G>
__global__ __launch_bounds__(KMC_TR_THREADS)
void kmc_trim_reduce_group_kernel(TrimBits B, const u64* __restrict__ offsets, u64 n_reads, u64 n_bases, int k, uint4* __restrict__ runs,
                                  const u32* __restrict__ list, kmc_ull* __restrict__ ctl) {
    __shared__ TrimRun part[KMC_TR_WAVES];
    constexpr int PER_WG = KMC_TR_THREADS / G;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = G == 64 ? lane : tid;
    u64 n_listed = ctl[G == 64 ? KMC_TR_N_WAVE : KMC_TR_N_GROUP];
    if (n_listed > n_reads) n_listed = n_reads;
    u64 n_bad = 0;   // member 0 counts for its group
    for (u64 i = (u64)blockIdx.x * PER_WG + (G == 64 ? wv : 0); i < n_listed; i += (u64)gridDim.x * PER_WG) {
        const u64 r = list[G == 64 ? i : n_reads - 1 - i];
        u64 a = 0, b = 0, bad = 0, lng = 0;
        const bool ok = r < n_reads && t_range(offsets, n_bases, k, r, a, b, bad, lng) && b > a;   // (uniform in the group)
        TrimRun e = t_none();
        if (ok) {
            const u64 w0 = a >> 6, n_w = ((b - 1) >> 6) + 1 - w0, per = (n_w + G - 1) / G;
            const u64 s0 = w0 + (u64)g * per, s1 = s0 + per;
            e = t_slice(B, a, b, s0 < w0 + n_w ? s0 : w0 + n_w, s1 < w0 + n_w ? s1 : w0 + n_w);
        }
        e = t_wave_join(e);
        if (G != 64) {
            if (lane == 0) part[wv] = e;
            __syncthreads();
            if (tid == 0) {
#pragma unroll
                for (int w = 1; w < KMC_TR_WAVES; ++w) e = t_join(e, part[w]);
            }
            __syncthreads();
        }
        if (g == 0) {
            if (ok) t_store(runs, r, e);
            else ++n_bad;   // (a listed read has windows and offsets that fit)
        }
    }
    if (g == 0 && n_bad) atomicAdd(&ctl[KMC_TR_BAD], (kmc_ull)n_bad);
}

struct TrimRule {
    int mode, k;
    u32 flags, min_permille;
    u64 min_strong, min_len;
};

// (start, len) of read r's span and its own PASS (kmc.h: SPAN, PASS); L: its bases
__device__ __forceinline__ bool t_pass(const TrimRule& R, const uint4* __restrict__ runs, u64 r, u64 L, u32& start, u32& len) {
    const uint4 x = runs[2 * r], y = runs[2 * r + 1];
    const u64 V = x.x, S = x.y;
    start = 0; len = 0;
    if (R.mode == KMC_TR_MODE_NONE) len = (u32)L;
    else if (S > 0 && R.mode == KMC_TR_MODE_ENDS) { start = x.z; len = x.w - x.z + (u32)R.k; }
    else if (S > 0) { start = y.x; len = y.y + (u32)R.k - 1u; }
    return S >= R.min_strong && S * 1000ull >= (u64)R.min_permille * V && (u64)len >= R.min_len && (R.mode == KMC_TR_MODE_NONE || S > 0);
}

// One lane per read (grid stride): read_stats, verdict, emit[r] (0 / 1) and elen[r] (the emitted span's length, else 0)
__global__ __launch_bounds__(KMC_TR_THREADS)
void kmc_trim_verdict_kernel(TrimRule R, const uint4* __restrict__ runs, const u64* __restrict__ offsets, u64 n_reads, u64 n_bases,
                             uint4* __restrict__ read_stats, uint8_t* __restrict__ verdict, u32* __restrict__ emit, u32* __restrict__ elen,
                             kmc_ull* __restrict__ ctl) {
    u64 s_valid = 0, s_strong = 0, s_pass = 0, s_emit = 0, s_bases = 0, s_cut = 0, s_before = 0, n_bad = 0;
    for (u64 r = (u64)blockIdx.x * KMC_TR_THREADS + threadIdx.x; r < n_reads; r += (u64)gridDim.x * KMC_TR_THREADS) {
        const u64 o0 = offsets[r], o1 = offsets[r + 1];
        const u64 L = o1 >= o0 ? o1 - o0 : 0;   // (the reduce kernel has counted offsets that do not fit and reads too long)
        u32 start, len;
        const bool own = t_pass(R, runs, r, L, start, len);
        bool v = own;
        if (R.flags & (KMC_TR_PAIR_BOTH | KMC_TR_PAIR_EITHER)) {
            const u64 m = r ^ 1ull;
            bool mate = false;
            if (m < n_reads) {
                const u64 m0 = offsets[m], m1 = offsets[m + 1];
                u32 ms, ml;
                mate = t_pass(R, runs, m, m1 >= m0 ? m1 - m0 : 0, ms, ml);
            } else ++n_bad;   // (the host refuses an odd number of reads)
            v = (R.flags & KMC_TR_PAIR_BOTH) ? own && mate : own || mate;
        }
        const bool em = v != ((R.flags & KMC_TR_INVERT) != 0);
        if ((u64)start + len > L) { ++n_bad; len = 0; start = 0; }
        const uint4 x = runs[2 * r];
        read_stats[r] = make_uint4(x.x, x.y, start, len);
        verdict[r] = (uint8_t)((own ? 1u : 0u) | (em ? 2u : 0u));
        emit[r] = em ? 1u : 0u;
        elen[r] = em ? len : 0u;
        s_valid += x.x; s_strong += x.y; s_pass += own ? 1u : 0u; s_emit += em ? 1u : 0u;
        s_bases += em ? len : 0u; s_cut += em && (u64)len < L ? 1u : 0u; s_before += em ? L : 0ull;
    }
    const u64 t0 = wave_sum_u64(s_valid), t1 = wave_sum_u64(s_strong), t2 = wave_sum_u64(s_pass), t3 = wave_sum_u64(s_emit);
    const u64 t4 = wave_sum_u64(s_bases), t5 = wave_sum_u64(s_cut), t6 = wave_sum_u64(s_before), t7 = wave_sum_u64(n_bad);
    if ((threadIdx.x & 63) == 0) {
        if (t0) atomicAdd(&ctl[KMC_TR_VALID], (kmc_ull)t0);
        if (t1) atomicAdd(&ctl[KMC_TR_STRONG], (kmc_ull)t1);
        if (t2) atomicAdd(&ctl[KMC_TR_PASSED], (kmc_ull)t2);
        if (t3) atomicAdd(&ctl[KMC_TR_EMITTED], (kmc_ull)t3);
        if (t4) atomicAdd(&ctl[KMC_TR_BASES], (kmc_ull)t4);
        if (t5) atomicAdd(&ctl[KMC_TR_CUT], (kmc_ull)t5);
        if (t6) atomicAdd(&ctl[KMC_TR_BEFORE], (kmc_ull)t6);
        if (t7) atomicAdd(&ctl[KMC_TR_BAD], (kmc_ull)t7);
    }
}

// Behind the scans of emit (epos) and elen (lpos): out_offsets[n_out + 1], origin[n_out] and src[n_out], the batch position
// of each emitted span.  The arrays hold n_reads (+ 1) entries.  WHOLE: the spans are the reads themselves (src = offsets[r];
// kmc_normalize.hip.h, whose read_stats hold no span), else a span starts read_stats[r].z bases into its read.
template <bool WHOLE>
__global__ __launch_bounds__(KMC_TR_THREADS)
void kmc_trim_layout_kernel(const uint4* __restrict__ read_stats, const u64* __restrict__ offsets, u64 n_reads, const u32* __restrict__ emit,
                            const u32* __restrict__ elen, const u32* __restrict__ epos, const u32* __restrict__ lpos,
                            u64* __restrict__ out_offsets, u64* __restrict__ origin, u64* __restrict__ src, kmc_ull* __restrict__ ctl) {
    u64 n_bad = 0;
    for (u64 r = (u64)blockIdx.x * KMC_TR_THREADS + threadIdx.x; r < n_reads; r += (u64)gridDim.x * KMC_TR_THREADS) {
        const u64 i = epos[r];
        if (i + emit[r] > n_reads) { ++n_bad; continue; }
        if (emit[r]) {
            out_offsets[i] = lpos[r];
            origin[i] = r;
            src[i] = WHOLE ? offsets[r] : offsets[r] + read_stats[r].z;
        }
        if (r == n_reads - 1) out_offsets[i + emit[r]] = (u64)lpos[r] + elen[r];
    }
    const u64 sb = wave_sum_u64(n_bad);
    if ((threadIdx.x & 63) == 0 && sb) atomicAdd(&ctl[KMC_TR_BAD], (kmc_ull)sb);
}

// 16 bytes beginning `sh` bytes into the 32 bytes (lo, hi), as two 64-bit words
__device__ __forceinline__ void t_funnel(uint4 lo, uint4 hi, u32 sh, u64& x, u64& y) {
    const u64 w0 = (u64)lo.y << 32 | lo.x, w1 = (u64)lo.w << 32 | lo.z, w2 = (u64)hi.y << 32 | hi.x, w3 = (u64)hi.w << 32 | hi.z;
    const bool up = sh >= 8;
    const u64 a = up ? w1 : w0, b = up ? w2 : w1, c = up ? w3 : w2;
    const u32 s = (sh & 7u) * 8u;
    x = s ? (a >> s) | (b << (64 - s)) : a;
    y = s ? (b >> s) | (c << (64 - s)) : b;
}
// the first m (1..16) bytes of (x, y) moved up to byte j (j + m <= 16), the rest zero
__device__ __forceinline__ void t_place(u64& x, u64& y, u32 m, u32 j) {
    if (m < 8) { x &= (1ull << (8 * m)) - 1ull; y = 0; }
    else if (m < 16) y &= (1ull << (8 * (m - 8))) - 1ull;   // (m == 8: y = 0)
    if (j >= 8) { y = x << (8 * (j - 8)); x = 0; }
    else if (j) { y = y << (8 * j) | x >> (64 - 8 * j); x <<= 8 * j; }
}

// A lane per 16 aligned output bytes.  ctl[KMC_TR_N_OUT] / ctl[KMC_TR_N_BASES]: the scans' totals.  bases is readable to the
// next 16-byte boundary past n_bases (the batch's padding rule), out has room to the one past the emitted bases.  The block
// is filled span by span: the 16 bytes at a span's source position come from two aligned 16-byte loads and a funnel shift
// (the second load only where a byte of it is wanted), are cut to the bytes the span has in the block and moved into
// place.  One span fills most blocks; at most 16 have a byte in one.
__global__ __launch_bounds__(KMC_TR_THREADS)
void kmc_trim_gather_kernel(const uint8_t* __restrict__ bases, u64 n_bases, u64 n_reads, const u64* __restrict__ out_offsets,
                            const u64* __restrict__ src, uint8_t* __restrict__ out, kmc_ull* __restrict__ ctl) {
    const u64 n_out = ctl[KMC_TR_N_OUT], total = ctl[KMC_TR_N_BASES];
    const u64 p = ((u64)blockIdx.x * KMC_TR_THREADS + threadIdx.x) * 16;
    bool bad = n_out > n_reads || total > n_bases;
    if (!bad && p < total) {
        u64 lo = 0, hi = 0, o1 = p;   // (o1: where the span in hand ends; none yet)
        u64 s = 0;
        u32 j = 0;
#pragma unroll 1
        for (int seg = 0; seg < 16 && j < 16 && p + j < total; ++seg) {
            const u64 pos = p + j;
            // the emitted read of this byte: pos < total = out_offsets[n_out], and empty emitted reads are skipped by the search
            const u64 i = m_read_of(out_offsets, n_out, pos);
            if (i >= n_out) { bad = true; break; }
            o1 = out_offsets[i + 1];
            s = src[i] + (pos - out_offsets[i]);
            const u64 left = o1 - pos;
            const u32 m = left < 16 - j ? (u32)left : 16 - j;
            if (o1 <= pos || s + m > n_bases) { bad = true; break; }
            const u32 sh = (u32)(s & 15);
            const uint4* q = reinterpret_cast<const uint4*>(bases + (s - sh));
            const uint4 a = q[0];
            uint4 b = make_uint4(0, 0, 0, 0);
            if (sh + m > 16) b = q[1];
            u64 x, y;
            t_funnel(a, b, sh, x, y);
            t_place(x, y, m, j);
            lo |= x; hi |= y;
            j += m;
        }
        if (!bad) *reinterpret_cast<uint4*>(out + p) = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    }
    const u64 m = __builtin_amdgcn_ballot_w64(bad);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[KMC_TR_BAD], (kmc_ull)__popcll(m));
}
