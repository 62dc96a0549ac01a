// kmc_query.hip.h -- asking the count table questions, on the sorted view kmc_finalize left in HBM
// (include/kmc.h: kmc_query, kmc_query_device, kmc_profile, kmc_profile_device):
//
//   prefix index   idx[p] = lower bound of the keys whose top P significant bits equal p, p = 0..2^P (kmc_query_index_kernel)
//   key lookup     count of each given key, 0 if absent (kmc_query_kernel)
//   read profile   per base position the count of the window that STARTS there, per read five statistics (kmc_profile_kernel)
//
// A lookup is a chain of dependent gathers: one index read (idx[p] and idx[p + 1] in one 8-byte load) bounds the bucket,
// a binary search inside the bucket that stops at the first equal key finds the position (one trip for a bucket of one key,
// log2(bucket) + 1 at most, so a view whose keys all share one prefix stays correct), one load fetches the count.  Nothing
// here is bandwidth: what hides the latency is the number of independent chains in flight.  A lane therefore runs
// KMC_Q_U lookups in lock step -- every trip issues the loads of all of them before it looks at any -- and the kernels are
// small enough in registers to keep several waves per SIMD.
#pragma once
#include "kmc_device.hip.h"
#include "kmc_stream.hip.h"

#define KMC_Q_THREADS 256
#define KMC_Q_WAVES (KMC_Q_THREADS / 64)
#define KMC_Q_U 8                 // lookups a lane runs in lock step
#define KMC_Q_MAX_P 27            // index of at most 2^27 + 1 u32 entries (512 MiB), reached at 2^28 keys
#define KMC_PROF_INIT_THREADS 256

typedef u32 kmc_u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// The sorted view and its index as the kernels see them.  sh = key bits - P; a key above (max_hi, max_lo) -- more than
// the ctx's key bits -- is absent without a look (its prefix would lie outside the index).
struct QView : KView {
    u32* idx;
    int sh;
    u64 max_hi, max_lo;
};

// log2 of the index size for a view of n keys of kb bits: two keys per bucket on average while the cap allows
static inline int kmc_query_index_bits(u64 n, int kb) {
    int bl = 0;
    while (bl < 64 && (n >> bl)) ++bl;
    int P = bl > 1 ? bl - 1 : 0;
    if (P > KMC_Q_MAX_P) P = KMC_Q_MAX_P;
    if (P > kb) P = kb;
    return P;
}

// top P bits of the kb-bit key (sh = kb - P in 0..127, P <= 27)
template <int KW>
__device__ __forceinline__ u32 q_prefix(int sh, u64 hi, u64 lo) {
    if (KW == 1) return sh >= 64 ? 0u : (u32)(lo >> sh);
    if (sh >= 64) return (u32)(hi >> (sh - 64));
    if (sh == 0) return (u32)lo;
    return (u32)((hi << (64 - sh)) | (lo >> sh));
}

// One thread per view position i = 0..n (n itself stands for the end: prefix 2^P).  Position i fills the entries
// (prefix of key i-1, prefix of key i] with i: 2^P + 1 stores in all, whatever the skew.  A long gap (a view whose keys
// crowd into few buckets) is filled by the whole wave.
template <int KW>
__global__ __launch_bounds__(256)
void kmc_query_index_kernel(QView v, u32 n_prefix) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool act = i <= v.n;
    u32 from = 0, to = 0;   // entries [from, to)
    if (act) {
        to = (i < v.n ? q_prefix<KW>(v.sh, KW == 2 ? v.hi[i] : 0, v.lo[i]) : n_prefix) + 1u;
        from = i > 0 ? q_prefix<KW>(v.sh, KW == 2 ? v.hi[i - 1] : 0, v.lo[i - 1]) + 1u : 0u;
    }
    const bool big = to - from > 32u;
    if (!big) for (u32 p = from; p < to; ++p) v.idx[p] = (u32)i;
    u64 m = __builtin_amdgcn_ballot_w64(big);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const u32 f = __shfl(from, src), t = __shfl(to, src), val = __shfl((u32)i, src);
        for (u64 p = (u64)f + lane; p < t; p += 64) v.idx[p] = val;
    }
}

// U lookups of one lane in lock step: out[u] = count of key u, 0 if absent or !(okmask >> u & 1).
template <int KW, int U>
__device__ __forceinline__ void q_lookup(const QView& v, const u64 (&khi)[U], const u64 (&klo)[U], u32 okmask, u64 (&out)[U]) {
    u32 lo[U], hi[U];
    u32 found = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        kmc_u32x2_a4 b = {0u, 0u};
        if ((okmask >> u) & 1) b = *reinterpret_cast<const kmc_u32x2_a4*>(v.idx + q_prefix<KW>(v.sh, khi[u], klo[u]));
        lo[u] = b.x; hi[u] = b.y;
    }
    u32 live = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) live |= lo[u] < hi[u] ? 1u << u : 0u;
    while (__builtin_amdgcn_ballot_w64(live != 0) != 0) {
        u64 mlo[U], mhi[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32 mid = lo[u] + ((hi[u] - lo[u]) >> 1);
            mlo[u] = 0; mhi[u] = 0;
            if ((live >> u) & 1) {
                mlo[u] = v.lo[mid];
                if (KW == 2) mhi[u] = v.hi[mid];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if ((live >> u) & 1) {
                const u32 mid = lo[u] + ((hi[u] - lo[u]) >> 1);
                const bool eq = mlo[u] == klo[u] && (KW == 1 || mhi[u] == khi[u]);
                const bool less = KW == 1 ? mlo[u] < klo[u] : key_less(mhi[u], mlo[u], khi[u], klo[u]);
                if (eq) { lo[u] = mid; found |= 1u << u; live &= ~(1u << u); }
                else {
                    if (less) lo[u] = mid + 1; else hi[u] = mid;
                    if (lo[u] >= hi[u]) live &= ~(1u << u);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) out[u] = (found >> u) & 1 ? v.cnt[lo[u]] : 0ull;
}

// The same search for the POSITION: pos[u] = view row of key u, KMC_Q_NOPOS if absent or !(okmask >> u & 1)
// (kmc_unitig.hip.h: the row of a key's one neighbour).
#define KMC_Q_NOPOS 0xFFFFFFFFu
template <int KW, int U>
__device__ __forceinline__ void q_find(const QView& v, const u64 (&khi)[U], const u64 (&klo)[U], u32 okmask, u32 (&pos)[U]) {
    u32 lo[U], hi[U];
    u32 found = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        kmc_u32x2_a4 b = {0u, 0u};
        if ((okmask >> u) & 1) b = *reinterpret_cast<const kmc_u32x2_a4*>(v.idx + q_prefix<KW>(v.sh, khi[u], klo[u]));
        lo[u] = b.x; hi[u] = b.y;
    }
    u32 live = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) live |= lo[u] < hi[u] ? 1u << u : 0u;
    while (__builtin_amdgcn_ballot_w64(live != 0) != 0) {
        u64 mlo[U], mhi[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32 mid = lo[u] + ((hi[u] - lo[u]) >> 1);
            mlo[u] = 0; mhi[u] = 0;
            if ((live >> u) & 1) {
                mlo[u] = v.lo[mid];
                if (KW == 2) mhi[u] = v.hi[mid];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if ((live >> u) & 1) {
                const u32 mid = lo[u] + ((hi[u] - lo[u]) >> 1);
                const bool eq = mlo[u] == klo[u] && (KW == 1 || mhi[u] == khi[u]);
                const bool less = KW == 1 ? mlo[u] < klo[u] : key_less(mhi[u], mlo[u], khi[u], klo[u]);
                if (eq) { lo[u] = mid; found |= 1u << u; live &= ~(1u << u); }
                else {
                    if (less) lo[u] = mid + 1; else hi[u] = mid;
                    if (lo[u] >= hi[u]) live &= ~(1u << u);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) pos[u] = (found >> u) & 1 ? lo[u] : KMC_Q_NOPOS;
}

// count[i] = count of key i.  A wave takes 64 x KMC_Q_U consecutive keys: lane l the pairs 2 (r * 64 + l) + {0, 1}, r = 0..U/2-1,
// so every load and store instruction moves 1 KiB contiguous (16 bytes per lane) when the arrays are 16-byte aligned (al16);
// otherwise the same elements go word by word.  key_hi == nullptr: all high words are zero.
template <int KW>
__global__ __launch_bounds__(KMC_Q_THREADS)
void kmc_query_kernel(QView v, const u64* __restrict__ key_hi, const u64* __restrict__ key_lo, u64 n_keys, int al16,
                      u64* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * KMC_Q_WAVES + (threadIdx.x >> 6);
    const u64 base = wave * (64 * KMC_Q_U);
    if (base >= n_keys) return;
    u64 khi[KMC_Q_U], klo[KMC_Q_U], out[KMC_Q_U];
    u32 ok = 0;
#pragma unroll
    for (int r = 0; r < KMC_Q_U / 2; ++r) {
        const u64 e = base + 2 * ((u64)r * 64 + lane);
        kmc_ull2 l = {0ull, 0ull}, h = {0ull, 0ull};
        if (al16 && e + 1 < n_keys) {
            l = *reinterpret_cast<const kmc_ull2*>(key_lo + e);
            if (key_hi) h = *reinterpret_cast<const kmc_ull2*>(key_hi + e);
        } else {
            if (e < n_keys) { l.x = key_lo[e]; if (key_hi) h.x = key_hi[e]; }
            if (e + 1 < n_keys) { l.y = key_lo[e + 1]; if (key_hi) h.y = key_hi[e + 1]; }
        }
        klo[2 * r] = l.x; klo[2 * r + 1] = l.y; khi[2 * r] = h.x; khi[2 * r + 1] = h.y;
        if (e < n_keys && !key_less(v.max_hi, v.max_lo, h.x, l.x)) ok |= 1u << (2 * r);
        if (e + 1 < n_keys && !key_less(v.max_hi, v.max_lo, h.y, l.y)) ok |= 2u << (2 * r);
    }
    q_lookup<KW, KMC_Q_U>(v, khi, klo, ok, out);
#pragma unroll
    for (int r = 0; r < KMC_Q_U / 2; ++r) {
        const u64 e = base + 2 * ((u64)r * 64 + lane);
        if (al16 && e + 1 < n_keys) {
            const kmc_ull2 o = {out[2 * r], out[2 * r + 1]};
            *reinterpret_cast<kmc_ull2*>(count + e) = o;
        } else {
            if (e < n_keys) count[e] = out[2 * r];
            if (e + 1 < n_keys) count[e + 1] = out[2 * r + 1];
        }
    }
}

// ---- per-read profiles -----------------------------------------------------------------------------------------------------
// read_stats rows are [valid windows, windows with count >= threshold, min, max, sum]; the launch sets min to all ones so
// that atomicMin works, and kmc_profile_fix_kernel puts 0 there for reads without a valid window.
#define KMC_PROFILE_STAT_WORDS 5
__global__ __launch_bounds__(KMC_PROF_INIT_THREADS)
void kmc_profile_init_kernel(kmc_ull* __restrict__ rs, u64 n_reads) {
    const u64 i = (u64)blockIdx.x * KMC_PROF_INIT_THREADS + threadIdx.x;
    if (i < n_reads * KMC_PROFILE_STAT_WORDS) rs[i] = (i % KMC_PROFILE_STAT_WORDS) == 2 ? ~0ull : 0ull;
}
__global__ __launch_bounds__(KMC_PROF_INIT_THREADS)
void kmc_profile_fix_kernel(kmc_ull* __restrict__ rs, u64 n_reads) {
    const u64 r = (u64)blockIdx.x * KMC_PROF_INIT_THREADS + threadIdx.x;
    if (r < n_reads && rs[r * KMC_PROFILE_STAT_WORDS] == 0) rs[r * KMC_PROFILE_STAT_WORDS + 2] = 0;
}

struct ProfAcc {
    u32 nv, np;
    u64 mn, mx, sm;
    __device__ __forceinline__ void clear() { nv = 0; np = 0; mn = ~0ull; mx = 0; sm = 0; }
    __device__ __forceinline__ void add(u64 c, u64 thr) {
        nv += 1; np += c >= thr ? 1u : 0u;
        mn = c < mn ? c : mn; mx = c > mx ? c : mx; sm += c;
    }
    __device__ __forceinline__ void merge(const ProfAcc& o) {
        nv += o.nv; np += o.np;
        mn = o.mn < mn ? o.mn : mn; mx = o.mx > mx ? o.mx : mx; sm += o.sm;
    }
    __device__ __forceinline__ void flush(kmc_ull* __restrict__ rs, u64 rid) const {
        if (!nv) return;
        kmc_ull* row = rs + rid * KMC_PROFILE_STAT_WORDS;
        atomicAdd(&row[0], (kmc_ull)nv);
        if (np) atomicAdd(&row[1], (kmc_ull)np);
        atomicMin(&row[2], (kmc_ull)mn);
        if (mx) atomicMax(&row[3], (kmc_ull)mx);
        if (sm) atomicAdd(&row[4], (kmc_ull)sm);
    }
};

struct ProfLds {
    u32 sbits[KMC_Q_WAVES][64];
    u32 tr[KMC_Q_WAVES][1024];
};

// Chunks of 1024 positions, a wave walks chunks_per_wave of them in order behind one warm-up chunk for the halo; per chunk a
// lane owns 16 positions.  Window extraction, validity (read starts, non-ACGT bytes) and canonical strand are the chunk
// front end's (kmc_chunks.hip.h, which describes the layout, the halo and the validity rule): it gives the key of the
// window ENDING at a position.  Its count is stored at the window's START, k - 1 positions earlier, through an LDS transpose
// (one store instruction = 256 contiguous bytes); invalid windows store 0, and n_chunks covers k - 1 positions past the
// batch's end, whose windows are all invalid: that is what zero-fills the last k - 1 slots of every read and of the batch.
// Per-read statistics: a lane folds its windows into runs of one read each (read index = reads starting at or before the
// position, found among the chunk's read starts); runs that end inside the lane go out with 64-bit atomics at once, the
// lane's last run is first combined with the neighbouring lanes' last runs of the same read (segmented reduction over the
// wave).  Reads longer than a chunk or a wave's span meet in the atomics, so every word is exact.
template <int KW, bool CANON>
__global__ __launch_bounds__(KMC_Q_THREADS)
void kmc_profile_kernel(const uint8_t* __restrict__ bases, u64 n_bases, const u64* __restrict__ offsets, u64 n_reads, int k,
                        u64 n_chunks, u64 chunks_per_wave, QView v, u64 thr, u32* __restrict__ window_count,
                        kmc_ull* __restrict__ read_stats) {
    constexpr int NW = 2 * KW + 1;  // window words: own + 2*KW preceding lanes
    __shared__ ProfLds L;
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
        W.step(bases, n_bases, c, true, L.sbits[wv]);
        if (c >= c0) {
            u32 X[NW], Yp[NW + 1];
            const u32 inv16 = chunk_windows<KW>(W, k, X);
            chunk_rc_stream<KW, CANON>(K, X, Yp);
            u64 cnt16[16];
#pragma unroll
            for (int h = 0; h < 16 / KMC_Q_U; ++h) {
                u64 khi[KMC_Q_U], klo[KMC_Q_U], out[KMC_Q_U];
#pragma unroll
                for (int u = 0; u < KMC_Q_U; ++u) chunk_key<KW, CANON>(K, X, Yp, KMC_Q_U * h + u, khi[u], klo[u]);
                q_lookup<KW, KMC_Q_U>(v, khi, klo, (~inv16 >> (KMC_Q_U * h)) & ((1u << KMC_Q_U) - 1u), out);
#pragma unroll
                for (int u = 0; u < KMC_Q_U; ++u) cnt16[KMC_Q_U * h + u] = out[u];
            }
            if (window_count) {
                u32* tr = L.tr[wv];
#pragma unroll
                for (int j = 0; j < 16; ++j) tr[lane * 16 + ((j + lane) & 15)] = cnt16[j] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)cnt16[j];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = 4 * i + (lane >> 4), col = lane & 15;
                    const u32 x = tr[row * 16 + ((col + row) & 15)];
                    const u64 endp = W.cb + 64u * i + lane;   // the window ends here and starts k - 1 earlier
                    if (endp + 1 >= (u64)k && endp + 1 - (u64)k < n_bases) window_count[endp + 1 - (u64)k] = x;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            if (read_stats && __builtin_amdgcn_ballot_w64((~inv16 & 0xFFFFu) != 0) != 0) {
                // read of this lane's first position: offsets[0 .. r_first) lie before the chunk
                u64 a = W.r_first, b = W.r_end;
                while (a < b) {
                    const u64 mid = (a + b) >> 1;
                    if (offsets[mid] <= W.pp) a = mid + 1; else b = mid;
                }
                u64 rid = a - 1;   // (pp < n_bases has offsets[0] = 0 <= pp; lanes past the end hold no valid window)
                ProfAcc acc;
                acc.clear();
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (j > 0 && ((W.st >> j) & 1)) {   // reads start here (several, if empty ones lie between)
                        acc.flush(read_stats, rid);
                        acc.clear();
                        while (rid + 1 < W.r_end && offsets[rid + 1] <= W.pp + j) ++rid;
                    }
                    if (!((inv16 >> j) & 1)) acc.add(cnt16[j], thr);
                }
                // the lanes' last runs: read indices do not decrease along the wave, so "same read 2^s lanes further" means
                // the same read in between
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    ProfAcc t;
                    t.nv = __shfl_down(acc.nv, o); t.np = __shfl_down(acc.np, o);
                    t.mn = __shfl_down(acc.mn, o); t.mx = __shfl_down(acc.mx, o); t.sm = __shfl_down(acc.sm, o);
                    const u64 orid = __shfl_down(rid, o);
                    if (lane + o < 64 && orid == rid) acc.merge(t);
                }
                const u64 prid = __shfl_up(rid, 1);
                if (lane == 0 || prid != rid) acc.flush(read_stats, rid);
            }
        }
    }
}
