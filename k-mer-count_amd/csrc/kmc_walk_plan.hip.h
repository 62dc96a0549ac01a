// kmc_walk_plan.hip.h -- the rank plan of the walk path: a repeat batch is finalized by ONE small launch.
//
// What kmc_walk_tail_kernel and kmc_small_finalize_kernel do behind a walk launch -- unfold the dense traversal counters
// (gcnt, one total per snapshot slot) into table adds, read the table back, rank-sort it, publish -- recomputes, launch
// after launch, things that are pure functions of the memo snapshot: which k-mer an item (snapshot slot, step) stands for,
// and where that k-mer sorts among the others.  Only the 2,048 totals change from call to call.  The PLAN keeps both next
// to the memo:
//   rank[item]   the row of the item's k-mer in the sorted view the plan was built from, or SKIP (the item stands for no
//                k-mer: step past the label, context shorter than k), or NONE (no row: the entry did not exist when the
//                plan was built, or its k-mer was not in that view);
//   keys[P]      the P <= KMC_WALK_PLAN_MAX sorted keys the ranks refer to.
// kmc_walk_plan_build_kernel fills it from an ordinary finalize (the item -> key rule is walk_item_kmer / walk_key, the
// same code the unfold runs); kmc_walk_plan_finalize_kernel, one workgroup queued between the walk launch and its tail,
// gathers the totals into P counts in LDS, drops the zero rows, writes the view and publishes exactly what
// kmc_fin_publish_and_drain publishes -- if, and only if, the host has asked for this finalize by then and the launch left
// nothing outside the dense counters.  Otherwise it touches nothing but its status word and the two kernels behind it run
// as they always did.  No global atomic, no hash table, no sort; nobody waits for anybody.
#pragma once
#include "kmc_table.hip.h"
#include "kmc_walk.hip.h"

#define KMC_WALK_PLAN_MAX 4096          // rows: 32 KB of counts in LDS, four rows per thread of the one workgroup
#define KMC_WALK_PLAN_BUILDS 8          // plans built per source (kmc_forget_source starts a new one): a memo that keeps growing
                                        // does not rebuild forever
#define KMC_PLAN_SKIP 0xFFFFu
#define KMC_PLAN_NONE 0xFFFEu
// the plan launch's pinned words (the host's side of them: kmc_ctx::h_plan)
enum { KMC_PLAN_W_REQ = 0,      // host -> device: the number of the finalize the host has queued last (launch_small_finalize), if
                                // a plan launch was armed for exactly that number; else 0
       KMC_PLAN_W_STATUS = 1,   // device -> host: seq * 4 + what the plan launch numbered seq did
       KMC_PLAN_W_N = 8 };
enum { KMC_PLAN_DONE = 1, KMC_PLAN_STALE = 2, KMC_PLAN_DECLINED = 3 };
// where a plan finalize leaves its number for the kmc_small_finalize_kernel behind it: a u64 at ticket + KMC_FIN_TICKET_PLAN
// (kmc_table.hip.h; words 0..2 are the finalize's own, word 3 is kmc_reset_kernel's ticket)

struct WalkPlan {
    unsigned short* rank;   // KMC_WALK_ITEMS
    u64* keys_lo;           // KMC_WALK_PLAN_MAX
    u64* keys_hi;           // the same, two-word keys only
    u32 n;                  // rows
};

// One thread per item of the snapshot the last launch wrote; (vhi, vlo): the n sorted keys of the view just finalized.
template <int KW, bool CANON>
__global__ __launch_bounds__(256)
void kmc_walk_plan_build_kernel(const WalkMemoSlot<KW>* memo, int k, const u64* __restrict__ vhi, const u64* __restrict__ vlo, WalkPlan pl) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < pl.n) {
        pl.keys_lo[w] = vlo[w];
        if (KW == 2) pl.keys_hi[w] = vhi[w];
    }
    if (w >= KMC_WALK_ITEMS) return;
    const int kb = 2 * k;
    const u64 mask_lo = kb >= 64 ? ~0ull : ((1ull << kb) - 1);
    const u64 mask_hi = kb <= 64 ? 0ull : ((1ull << (kb - 64)) - 1);
    const u32 i = w / KMC_WALK_STRIDE, step = w % KMC_WALK_STRIDE;
    const bool valid = memo->tag == (KMC_WALK_MEMO_TAG | (u64)k);
    const bool exists = valid && (i < KMC_WALK_NCAP ? (memo->prim[i] >> 32) != 0 : memo->ekv[i - KMC_WALK_NCAP] != ~0ull);
    u32 r = KMC_PLAN_NONE;   // (an entry that appears later gets a counter: the plan launch then reports the plan stale)
    if (exists) {
        WCtx ctx;
        if (!walk_item_kmer<KW>(memo, i, step, k, mask_hi, mask_lo, ctx)) {
            r = KMC_PLAN_SKIP;
        } else {
            u64 khi, klo;
            walk_key<CANON>(ctx, k, khi, klo);
            u32 lo = 0, hi = pl.n;   // first row whose key is not smaller
            while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                const u64 mh = KW == 2 ? vhi[mid] : 0ull, ml = vlo[mid];
                if (KW == 2 ? (mh < khi || (mh == khi && ml < klo)) : ml < klo) lo = mid + 1; else hi = mid;
            }
            if (lo < pl.n && vlo[lo] == klo && (KW == 1 || vhi[lo] == khi)) r = lo;
        }
    }
    pl.rank[w] = (unsigned short)r;
}

// ONE workgroup of 1024 threads, between a walk launch and its tail.  Everything it reads to decide is stable at this point
// of the stream except the request word, which is read once.
template <int KW>
__global__ __launch_bounds__(1024)
void kmc_walk_plan_finalize_kernel(const WalkWs* ws, u64* gcnt, const WalkMemoSlot<KW>* memo, int k, WalkPlan pl, GTable g,
                                   const u64* __restrict__ sk_counters, u32* __restrict__ ticket, u64* __restrict__ host_mirror,
                                   u64* __restrict__ words, u64 seq, u64* __restrict__ out_hi, u64* __restrict__ out_lo, u64* __restrict__ out_cnt) {
    static_assert(KMC_WALK_ITEMS == 1024 * 32 && KMC_WALK_PLAN_MAX == 1024 * 4, "a thread takes two snapshot entries and four rows");
    __shared__ u64 s_cnt[KMC_WALK_PLAN_MAX];
    __shared__ u32 s_go;
    __shared__ u32 s_rows[16];
    __shared__ u64 s_sum[16];
    const u32 tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    // The kernel is a chain of memory round trips, not work: EVERYTHING it may read is requested here, at once, before the
    // decision -- a thread's 32 ranks (entries 2 tid and 2 tid + 1), their two totals, the keys of its four rows, the
    // counters it would publish, and in wave 0 the words the decision rests on, one per lane.  (Reads only: a launch that
    // declines has touched nothing.  Read one after the other by one thread, the decision words alone were 8 round trips.)
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t rk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) rk[q] = reinterpret_cast<const u32x4_t*>(pl.rank)[tid * 4 + q];
    const kmc_ull2 tot2 = reinterpret_cast<const kmc_ull2*>(gcnt)[tid];
    kmc_ull2 klo[2], khi[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        klo[q] = reinterpret_cast<const kmc_ull2*>(pl.keys_lo)[2 * tid + q];
        if (KW == 2) khi[q] = reinterpret_cast<const kmc_ull2*>(pl.keys_hi)[2 * tid + q];
    }
    u64 pub = 0;   // what this thread would publish
    if (tid < KMC_CTR_FINSEQ) pub = g.counters[tid];
    else if (tid >= 16 && tid < 16 + KMC_CTR_N) pub = sk_counters[tid - 16];
    u32 okn = 0, skn = 0;
    if (tid == KMC_CTR_FINSEQ) { okn = ticket[1]; skn = ticket[2]; pub = g.counters[KMC_CTR_SLABSKIP]; }
    if (tid < 64) {
        // (a) the host has queued the finalize this launch was armed for (the one word that may change: read once);
        // (b) nothing is in the count table -- not from this launch (entries it created itself, direct adds), not from
        // before -- and nothing pending in the (k+16)-mer table; (c) no read was diverted; (d) the launch ran from a snapshot
        bool good = true;
        if (lane == 0) good = __hip_atomic_load(&words[KMC_PLAN_W_REQ], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == seq;
        else if (lane == 1) good = g.counters[KMC_CTR_OCCUPIED] == 0;
        else if (lane == 2) good = g.counters[KMC_CTR_SPILL] == 0;
        else if (lane == 3) good = g.counters[KMC_CTR_ERR] == 0;
        else if (lane == 4) good = sk_counters[KMC_CTR_KMERS] == 0;
        else if (lane == 5) good = ws->n_deferred == 0;
        else if (lane == 6) good = memo->tag == (KMC_WALK_MEMO_TAG | (u64)k);
        else if (lane == 7) good = pl.n <= KMC_WALK_PLAN_MAX;
        const bool go = __builtin_amdgcn_ballot_w64(!good) == 0;
        if (lane == 0) {
            s_go = go ? 1u : 0u;
            if (!go) __hip_atomic_store(&words[KMC_PLAN_W_STATUS], seq * 4 + KMC_PLAN_DECLINED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s_cnt[tid + 1024 * j] = 0;
    __syncthreads();
    if (!s_go) return;
    // every item's total into its row
    bool stale = false;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const u64 tot = tot2[e];
        if (tot) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const u32 word = rk[2 * e + (j >> 3)][(j >> 1) & 3];
                const u32 r = (j & 1) ? word >> 16 : word & 0xFFFFu;
                if (r == KMC_PLAN_SKIP) continue;
                if (r >= pl.n) stale = true;   // (NONE, or a row the plan does not have)
                else atomicAdd((kmc_ull*)&s_cnt[r], (kmc_ull)tot);
            }
        }
    }
    // (e) a counter on an item the plan has no row for: the memo has grown, or this batch holds k-mers the plan's did not
    if (__syncthreads_or(stale ? 1 : 0)) {
        if (tid == 0) __hip_atomic_store(&words[KMC_PLAN_W_STATUS], seq * 4 + KMC_PLAN_STALE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    // from here on the launch IS the finalize.  Rows 4 tid .. 4 tid + 3: keep the nonzero ones, in order
    u64 c4[4];
    u32 mine = 0;
    u64 sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c4[j] = s_cnt[4 * tid + j]; mine += c4[j] ? 1u : 0u; sum += c4[j]; }
    u32 incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const u32 v = __shfl_up(incl, d); if (lane >= (u32)d) incl += v; }
    sum = wave_sum_u64(sum);
    if (lane == 63) s_rows[wv] = incl;
    if (lane == 0) s_sum[wv] = sum;
    __syncthreads();
    u32 pos = incl - mine, rows = 0;
    u64 total = 0;
    for (u32 w = 0; w < 16; ++w) { if (w < wv) pos += s_rows[w]; rows += s_rows[w]; total += s_sum[w]; }
    // publish what kmc_fin_publish_and_drain publishes (kmc_table.hip.h): the counters, OCCUPIED = the rows of the view,
    // SUM2 = the sum of their counts, the verdict, FINSEQ last behind the system fence.  The host is told FIRST: what
    // follows -- the view's rows among it -- is device memory, in stream order before whatever the host queues next, and
    // anybody outside the stream gets the view from kmc_export_device, which waits for the end of this kernel (poll_fin:
    // view_unsynced); the fence then waits for a dozen words, not for the view.
    if (tid == KMC_CTR_OCCUPIED)
        __hip_atomic_store(&host_mirror[tid], (u64)rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (tid < KMC_CTR_FINSEQ && tid != KMC_CTR_SUM2 && tid != KMC_CTR_FASTFIN)
        __hip_atomic_store(&host_mirror[tid], pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (tid == KMC_CTR_FINSEQ) {
        okn += 1u;
        skn += (u32)pub;
        __hip_atomic_store(&host_mirror[KMC_CTR_FINOK], (u64)okn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&host_mirror[KMC_CTR_FINSKIP], (u64)skn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&host_mirror[KMC_CTR_SUM2], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&host_mirror[KMC_CTR_FASTFIN], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&words[KMC_PLAN_W_STATUS], seq * 4 + KMC_PLAN_DONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    else if (tid >= 16 && tid < 16 + KMC_CTR_N)
        __hip_atomic_store(&host_mirror[KMC_CTR_N + tid - 16], pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // (every word above was stored by wave 0: its fence alone orders them in front of FINSEQ -- no barrier, and not sixteen
    // system-scope releases)
    static_assert(16 + KMC_CTR_N <= 64 && KMC_CTR_FINSEQ < 16, "wave 0 publishes");
    if (wv == 0) {
        __threadfence_system();
        if (lane == 0) __hip_atomic_store(&host_mirror[KMC_CTR_FINSEQ], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // the view, the dense counters as the tail would leave them, the device counters as a drain leaves them
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c4[j]) {
            out_lo[pos] = klo[j >> 1][j & 1];
            if (KW == 2) out_hi[pos] = khi[j >> 1][j & 1];
            out_cnt[pos] = c4[j];
            pos++;
        }
    }
    reinterpret_cast<kmc_ull2*>(gcnt)[tid] = kmc_ull2{0ull, 0ull};
    if (tid >= 64 && tid < 64 + KMC_CTR_N) g.counters[tid - 64] = 0;   // (read at the top of the kernel)
    if (tid == KMC_CTR_FINSEQ) { ticket[1] = okn; ticket[2] = skn; }
    if (tid == 0) *reinterpret_cast<u64*>(ticket + KMC_FIN_TICKET_PLAN) = seq;
}

// ---- host side ------------------------------------------------------------------------------
static inline int kmc_walk_plan_build_launch(hipStream_t st, int KW, int k, bool canon, const void* memo_slot, const u64* vhi, const u64* vlo, WalkPlan pl) {
    const dim3 grid(KMC_WALK_ITEMS / 256), block(256);
    if (KW == 1) {
        if (canon) hipLaunchKernelGGL((kmc_walk_plan_build_kernel<1, true>), grid, block, 0, st, (const WalkMemoSlot<1>*)memo_slot, k, vhi, vlo, pl);
        else hipLaunchKernelGGL((kmc_walk_plan_build_kernel<1, false>), grid, block, 0, st, (const WalkMemoSlot<1>*)memo_slot, k, vhi, vlo, pl);
    } else {
        if (canon) hipLaunchKernelGGL((kmc_walk_plan_build_kernel<2, true>), grid, block, 0, st, (const WalkMemoSlot<2>*)memo_slot, k, vhi, vlo, pl);
        else hipLaunchKernelGGL((kmc_walk_plan_build_kernel<2, false>), grid, block, 0, st, (const WalkMemoSlot<2>*)memo_slot, k, vhi, vlo, pl);
    }
    return hipGetLastError() == hipSuccess ? KMC_OK : KMC_ERR_HIP;
}
// `memo` / `parity`: as given to the walk launch in front (the snapshot slot it READ); ws: its workspace
static inline int kmc_walk_plan_finalize_launch(hipStream_t st, int KW, int k, void* ws, void* memo, int parity, WalkPlan pl, GTable g, const u64* sk_counters,
                                                u32* ticket, u64* host_mirror, u64* words, u64 seq, u64* out_hi, u64* out_lo, u64* out_cnt) {
    const WalkWs* hdr = (const WalkWs*)ws;
    u64* gcnt = (u64*)((char*)ws + sizeof(WalkWs));
    if (KW == 1) hipLaunchKernelGGL(kmc_walk_plan_finalize_kernel<1>, dim3(1), dim3(1024), 0, st, hdr, gcnt, (const WalkMemoSlot<1>*)memo + parity, k, pl, g, sk_counters,
                                    ticket, host_mirror, words, seq, out_hi, out_lo, out_cnt);
    else hipLaunchKernelGGL(kmc_walk_plan_finalize_kernel<2>, dim3(1), dim3(1024), 0, st, hdr, gcnt, (const WalkMemoSlot<2>*)memo + parity, k, pl, g, sk_counters,
                            ticket, host_mirror, words, seq, out_hi, out_lo, out_cnt);
    return hipGetLastError() == hipSuccess ? KMC_OK : KMC_ERR_HIP;
}
