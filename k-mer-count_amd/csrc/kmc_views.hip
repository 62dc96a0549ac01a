// kmc_views.hip -- the calls of include/kmc.h that only READ the sorted view a finalize left in HBM.  From the counting
// side (kmc_api.hip) they need resolve_view and the ctx (kmc_ctx.hip.h).
#include <stdlib.h>

#include <type_traits>

#include "kmc_ctx.hip.h"
#include "kmc_scan.hip.h"
#include "kmc_partition.hip.h"
#include "kmc_spectrum.hip.h"
#include "kmc_query.hip.h"
#include "kmc_setops.hip.h"
#include "kmc_graph.hip.h"
#include "kmc_unitig.hip.h"
#include "kmc_links.hip.h"
#include "kmc_clean.hip.h"
#include "kmc_components.hip.h"
#include "kmc_bubbles.hip.h"
#include "kmc_map.hip.h"
#include "kmc_transits.hip.h"
#include "kmc_pairs.hip.h"
#include "kmc_correct.hip.h"
#include "kmc_trim.hip.h"
#include "kmc_contigs.hip.h"
#include "kmc_normalize.hip.h"

namespace {

// the ctx's key words, and whether it counts canonical k-mers, as compile-time constants of a generic lambda
template <typename F>
void with_kw(const kmc_ctx* c, F&& f) {
    if (c->KW == 1) f(std::integral_constant<int, 1>{}); else f(std::integral_constant<int, 2>{});
}
template <typename F>
void with_kw_canon(const kmc_ctx* c, F&& f) {
    with_kw(c, [&](auto KW) { if (c->cfg.canonical) f(KW, std::true_type{}); else f(KW, std::false_type{}); });
}

// the sorted view of the last finalize (no high words for one-word keys)
KView view_of(const kmc_ctx* c) {
    return KView{c->KW == 2 ? c->v_hi : nullptr, c->v_lo, c->v_cnt, c->n_sorted};
}

// the kernels that read two entries per 16-byte load ask for this (an empty view has no arrays to speak of)
bool view_aligned16(const KView& v) { return !v.n || (((uintptr_t)v.hi | (uintptr_t)v.lo | (uintptr_t)v.cnt) & 15) == 0; }

// upper end of a count range: 0 stands for "no upper bound"
u64 count_hi(uint64_t max_count) { return max_count ? (u64)max_count : ~0ull; }

// the view is about to be read outside the ctx's stream order: a finalize that poll_fin saw done before it ended is waited for
int sync_view(kmc_ctx* c) {
    if (!c->view_unsynced) return KMC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->view_unsynced = false;
    return KMC_OK;
}

// What the calls that read the view check first: resolve_view, the count range (max_count != 0), that there is a view
int view_begin(kmc_ctx* c, const char* what, uint64_t min_count = 0, uint64_t max_count = 0) {
    if (int rc = resolve_view(c)) return rc;
    if (max_count && min_count > max_count)
        return fail(c, KMC_ERR_ARG, "%s: min_count %llu > max_count %llu", what, (unsigned long long)min_count, (unsigned long long)max_count);
    if (!c->sorted_valid) return fail(c, KMC_ERR_STATE, "%s before kmc_finalize", what);
    return KMC_OK;
}

// n entries of a table on the device queued into the caller's arrays (each optional; key_hi: zeros for one-word keys)
int queue_to_host(kmc_ctx* c, const void* hi, const void* lo, const void* cnt, u64 n, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count) {
    if (key_lo) HIPCHK(c, hipMemcpyAsync(key_lo, lo, n * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (count) HIPCHK(c, hipMemcpyAsync(count, cnt, n * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (key_hi) {
        if (c->KW == 2) HIPCHK(c, hipMemcpyAsync(key_hi, hi, n * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        else memset(key_hi, 0, n * sizeof(u64));
    }
    return KMC_OK;
}
// ... and waited for
int copy_to_host(kmc_ctx* c, const void* hi, const void* lo, const void* cnt, u64 n, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count) {
    if (int rc = queue_to_host(c, hi, lo, cnt, n, key_hi, key_lo, count)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KMC_OK;
}

// Scratch of an order-preserving compaction of n_tiles tiles -- counts (c_tile), their scan (c_tpos), block sums -- and
// ctl_words zeroed control words (c_ctl): word 0 takes the scan's total (a u32), the rest are the caller's.
int compact_plan(kmc_ctx* c, u64 n_tiles, u32 ctl_words) {
    const size_t nb = (size_t)((n_tiles + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK);
    int rc;
    if ((rc = ensure(c, c->c_tile, (size_t)n_tiles * sizeof(u32))) || (rc = ensure(c, c->c_tpos, (size_t)n_tiles * sizeof(u32))) ||
        (rc = ensure(c, c->c_bsum, (nb + 2) * sizeof(u32))) || (rc = ensure(c, c->c_ctl, ctl_words * sizeof(u64))))
        return rc;
    HIPCHK(c, hipMemsetAsync(c->c_ctl.p, 0, ctl_words * sizeof(u64), c->stream));
    return KMC_OK;
}
// behind the caller's count kernel: the scan of c_tile into c_tpos, its total into control word 0, then the control words
// into h[ctl_words]; waits for them
int compact_scan_and_read(kmc_ctx* c, u64 n_tiles, u64* h, u32 ctl_words) {
    launch_exclusive_scan<0>(c->stream, c->c_tile.p, (u32)n_tiles, (u32*)c->c_bsum.p, (u32*)c->c_tpos.p, (u32*)c->c_ctl.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h, c->c_ctl.p, ctl_words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KMC_OK;
}

}  // namespace

// ---- export and owner partition ----
static int kmc_export_impl(kmc_ctx* c, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap) {
    if (!c) return KMC_ERR_ARG;
    { int rc = view_begin(c, "kmc_export"); if (rc) return rc; }
    const u64 n = c->n_sorted;
    if (cap < n) return fail(c, KMC_ERR_ARG, "export capacity %llu < %llu distinct keys", (unsigned long long)cap, (unsigned long long)n);
    if (!n) return KMC_OK;
    if (!key_lo || !count) return fail(c, KMC_ERR_ARG, "null buffer");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return copy_to_host(c, c->v_hi, c->v_lo, c->v_cnt, n, key_hi, key_lo, count);
}

static int kmc_export_device_impl(kmc_ctx* c, const void** d_key_hi, const void** d_key_lo, const void** d_count, uint64_t* n_distinct) {
    if (!c) return KMC_ERR_ARG;
    int rc;
    if ((rc = view_begin(c, "kmc_export_device")) || (rc = sync_view(c))) return rc;
    const KView v = view_of(c);
    if (d_key_hi) *d_key_hi = v.hi;
    if (d_key_lo) *d_key_lo = v.lo;
    if (d_count) *d_count = v.cnt;
    if (n_distinct) *n_distinct = v.n;
    return KMC_OK;
}

extern "C" uint32_t kmc_owner_of(uint64_t key_hi, uint64_t key_lo, uint32_t n_parts) { return kmc_owner(key_hi, key_lo, n_parts); }

static int kmc_partition_device_impl(kmc_ctx* c, uint32_t n_parts, uint64_t* part_begin, const void** d_key_hi,
                                    const void** d_key_lo, const void** d_count) {
    if (!c || !n_parts || !part_begin) return KMC_ERR_ARG;
    { int rc = view_begin(c, "kmc_partition_device"); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const KView v = view_of(c);
    const u64 n = v.n;
    int rc;
    if ((rc = ensure_keys(c, c->p, n)) || (rc = ensure(c, c->t_idx0, (size_t)std::max<u64>(n_parts, 1) * sizeof(u64)))) return rc;
    if (n_parts > 4096) return fail(c, KMC_ERR_ARG, "kmc_partition_device: more than 4096 parts");
    std::vector<unsigned long long> cnt((size_t)n_parts, 0ull);
    unsigned long long* d_cnt = (unsigned long long*)c->t_idx0.p;  // (scratch: n_parts counters, then cursors)
    if (n) {
        const int g2 = grid_for(c, n, 256);
        HIPCHK(c, hipMemsetAsync(d_cnt, 0, (size_t)n_parts * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(kmc_owner_count_kernel, dim3(g2), dim3(256), (size_t)n_parts * sizeof(unsigned int), c->stream, v.hi, v.lo, n, n_parts, d_cnt);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n_parts * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    u64 pos = 0;
    std::vector<unsigned long long> cursor((size_t)n_parts);
    for (u32 p = 0; p < n_parts; ++p) { part_begin[p] = pos; cursor[p] = pos; pos += cnt[p]; }
    part_begin[n_parts] = pos;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(d_cnt, cursor.data(), (size_t)n_parts * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(kmc_owner_scatter_kernel, dim3(grid_for(c, n, 256)), dim3(256), 0, c->stream, v.hi, v.lo, v.cnt, n, n_parts, d_cnt,
                           (u64*)c->p.hi.p, (u64*)c->p.lo.p, (u64*)c->p.cnt.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (cursor[] is host memory of this call)
    }
    publish_keys(c, c->p, d_key_hi, d_key_lo, d_count);
    return KMC_OK;
}

// ---- abundance histogram and count-range filter of the sorted view (kmc_spectrum.hip.h) ----
static bool filter_is_identity(uint64_t min_count, uint64_t max_count) { return min_count <= 1 && max_count == 0; }

static int kmc_histogram_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint32_t n_bins, uint64_t* hist, uint64_t* max_seen) {
    if (!c) return KMC_ERR_ARG;
    int rc = view_begin(c, "kmc_histogram", min_count, max_count);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n_bins < 2 || n_bins > (1u << 24)) return fail(c, KMC_ERR_ARG, "kmc_histogram: n_bins %u outside 2..2^24", n_bins);
    if (!hist) return fail(c, KMC_ERR_ARG, "kmc_histogram: null histogram");
    const u64 n = c->n_sorted;
    if (!n) {
        memset(hist, 0, (size_t)n_bins * sizeof(u64));
        if (max_seen) *max_seen = 0;
        return KMC_OK;
    }
    rc = ensure(c, c->h_hist, ((size_t)n_bins + 1) * sizeof(u64));   // [hist | max]
    if (rc) return rc;
    kmc_ull* d = (kmc_ull*)c->h_hist.p;
    HIPCHK(c, hipMemsetAsync(d, 0, ((size_t)n_bins + 1) * sizeof(u64), c->stream));
    const u32 lds_bins = std::min<u32>(n_bins, KMC_SPEC_LDS_BINS);
    const u32 head = ((uintptr_t)c->v_cnt & 15) ? 1u : 0u;
    const u64 n_pairs = (n - head) / 2;
    // 64 KiB of LDS: two workgroups per CU (160 KiB); smaller histograms four.  No more workgroups than there are
    // pairs for: each one clears and flushes its whole LDS part.
    const u64 per_cu = (u64)lds_bins * sizeof(u32) > 40960 ? 2 : 4;
    const u64 grid = std::max<u64>(1, std::min<u64>((u64)c->n_cu * per_cu, (n_pairs + 2 * KMC_SPEC_THREADS - 1) / (2 * KMC_SPEC_THREADS)));
    hipLaunchKernelGGL(kmc_histogram_kernel, dim3((u32)grid), dim3(KMC_SPEC_THREADS), (size_t)lds_bins * sizeof(u32), c->stream,
                       c->v_cnt, n, head, (u64)min_count, count_hi(max_count), n_bins, lds_bins, d, d + n_bins);
    HIPCHK(c, hipGetLastError());
    u64 mx = 0;
    HIPCHK(c, hipMemcpyAsync(hist, d, (size_t)n_bins * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&mx, d + n_bins, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (max_seen) *max_seen = mx;
    return KMC_OK;
}

// reduce half of the filter: kept entries per tile, their exclusive scan (c_tpos), n_kept and the sum of kept counts
static int filter_count(kmc_ctx* c, u64 lo_c, u64 hi_c, u64* n_kept, u64* kept_total) {
    const KView v = view_of(c);
    *n_kept = *kept_total = 0;
    if (!v.n) return KMC_OK;
    if (!view_aligned16(v)) return fail(c, KMC_ERR_HIP, "internal error: sorted view not 16-byte aligned");
    const u64 n_tiles = (v.n + KMC_FILT_TILE - 1) / KMC_FILT_TILE;   // (n < 2^32: at most 2^21 tiles)
    int rc = compact_plan(c, n_tiles, 2);   // [n_kept | kept_total]
    if (rc) return rc;
    const u32 cgrid = (u32)std::min<u64>(n_tiles, (u64)c->n_cu * 8);
    hipLaunchKernelGGL(kmc_filter_count_kernel, dim3(cgrid), dim3(KMC_FILT_THREADS), 0, c->stream, v.cnt, v.n, n_tiles, lo_c, hi_c,
                       (u32*)c->c_tile.p, (kmc_ull*)c->c_ctl.p + 1);
    u64 h[2] = {0, 0};
    if ((rc = compact_scan_and_read(c, n_tiles, h, 2))) return rc;
    *n_kept = h[0];
    *kept_total = h[1];
    return KMC_OK;
}

// scatter half: the kept entries into the filter's result at tile base + wave offset + lane prefix (filter_count ran first);
// finished when it returns (kmc_export_device's ordering contract)
static int filter_scatter(kmc_ctx* c, u64 lo_c, u64 hi_c, u64 n_kept) {
    if (int rc = ensure_keys(c, c->f, n_kept)) return rc;
    if (!n_kept) return KMC_OK;
    const KView v = view_of(c);
    const u64 n_tiles = (v.n + KMC_FILT_TILE - 1) / KMC_FILT_TILE;
    with_kw(c, [&](auto KW) {
        hipLaunchKernelGGL(kmc_filter_scatter_kernel<KW()>, dim3((u32)n_tiles), dim3(KMC_FILT_THREADS), 0, c->stream, v.hi, v.lo, v.cnt,
                           v.n, lo_c, hi_c, (const u32*)c->c_tpos.p, (u64*)c->f.hi.p, (u64*)c->f.lo.p, (u64*)c->f.cnt.p);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KMC_OK;
}

static int kmc_filter_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void** d_key_hi, const void** d_key_lo,
                                  const void** d_count, uint64_t* n_kept, uint64_t* kept_total) {
    if (!c) return KMC_ERR_ARG;
    int rc = view_begin(c, "kmc_filter_device", min_count, max_count);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (filter_is_identity(min_count, max_count)) {   // keeps everything: the view itself, nothing launched
        uint64_t nd = 0;
        rc = kmc_export_device_impl(c, d_key_hi, d_key_lo, d_count, &nd);
        if (rc) return rc;
        if (n_kept) *n_kept = nd;
        if (kept_total) *kept_total = nd ? c->st.n_kmers : 0;
        return KMC_OK;
    }
    u64 nk = 0, kt = 0;
    if ((rc = filter_count(c, min_count, count_hi(max_count), &nk, &kt)) || (rc = filter_scatter(c, min_count, count_hi(max_count), nk))) return rc;
    publish_keys(c, c->f, d_key_hi, d_key_lo, d_count);
    if (n_kept) *n_kept = nk;
    if (kept_total) *kept_total = kt;
    return KMC_OK;
}

static int kmc_export_filtered_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t* key_hi, uint64_t* key_lo,
                                    uint64_t* count, uint64_t cap, uint64_t* n_kept) {
    if (!c) return KMC_ERR_ARG;
    if (n_kept) *n_kept = 0;
    int rc = view_begin(c, "kmc_export_filtered", min_count, max_count);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const bool ident = filter_is_identity(min_count, max_count);
    u64 nk = c->n_sorted, kt = 0;
    if (!ident) { rc = filter_count(c, min_count, count_hi(max_count), &nk, &kt); if (rc) return rc; }
    if (n_kept) *n_kept = nk;
    if (cap < nk) return fail(c, KMC_ERR_ARG, "kmc_export_filtered: capacity %llu < %llu kept keys", (unsigned long long)cap, (unsigned long long)nk);
    if (!nk) return KMC_OK;
    if (!key_lo || !count) return fail(c, KMC_ERR_ARG, "null buffer");
    if (ident) return kmc_export_impl(c, key_hi, key_lo, count, cap);
    rc = filter_scatter(c, min_count, count_hi(max_count), nk);
    if (rc) return rc;
    return copy_to_host(c, c->f.hi.p, c->f.lo.p, c->f.cnt.p, nk, key_hi, key_lo, count);
}

// ---- key lookups and per-read profiles against the sorted view (kmc_query.hip.h) ----
// The view as the query kernels see it, its prefix index built first if this view has none yet (one launch; kept until the
// ctx publishes another view).  An empty view gets an index of one empty bucket, so the kernels need no special case.
static int query_view(kmc_ctx* c, const char* what, QView* out) {
    const u64 n = c->n_sorted;
    if (n >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: a view of 2^32 keys or more cannot be indexed", what);
    const int kb = 2 * c->klen;
    const int P = kmc_query_index_bits(n, kb);
    QView v;
    static_cast<KView&>(v) = view_of(c);
    v.sh = kb - P;
    v.max_lo = kb >= 64 ? ~0ull : (1ull << kb) - 1;
    v.max_hi = kb <= 64 ? 0ull : (1ull << (kb - 64)) - 1;
    if (c->q_gen != c->view_gen || !c->q_idx.p) {
        int rc = ensure(c, c->q_idx, (((size_t)1 << P) + 2) * sizeof(u32));
        if (rc) return rc;
        v.idx = (u32*)c->q_idx.p;
        const u32 grid = (u32)((n + 1 + 255) / 256);
        with_kw(c, [&](auto KW) { hipLaunchKernelGGL(kmc_query_index_kernel<KW()>, dim3(grid), dim3(256), 0, c->stream, v, 1u << P); });
        HIPCHK(c, hipGetLastError());
        c->q_gen = c->view_gen;
    }
    v.idx = (u32*)c->q_idx.p;
    *out = v;
    return KMC_OK;
}

// the lookup launch (device arrays; d_hi may be null: high words zero)
static int query_launch(kmc_ctx* c, const u64* d_hi, const u64* d_lo, u64 n_keys, u64* d_cnt) {
    QView v;
    if (int rc = query_view(c, "kmc_query", &v)) return rc;
    const int al16 = (((uintptr_t)d_hi | (uintptr_t)d_lo | (uintptr_t)d_cnt) & 15) == 0;
    const u64 per_wg = (u64)KMC_Q_THREADS * KMC_Q_U;
    const u64 grid = (n_keys + per_wg - 1) / per_wg;
    if (grid > 0x7FFFFFFFull) return fail(c, KMC_ERR_ARG, "kmc_query: too many keys in one call");
    with_kw(c, [&](auto KW) {
        hipLaunchKernelGGL(kmc_query_kernel<KW()>, dim3((u32)grid), dim3(KMC_Q_THREADS), 0, c->stream, v, d_hi, d_lo, n_keys, al16, d_cnt);
    });
    HIPCHK(c, hipGetLastError());
    return KMC_OK;
}

static int kmc_query_device_impl(kmc_ctx* c, const void* d_key_hi, const void* d_key_lo, uint64_t n_keys, void* d_count) {
    if (!c) return KMC_ERR_ARG;
    if (int rc = view_begin(c, "kmc_query_device")) return rc;
    if (!n_keys) return KMC_OK;
    if (!d_key_lo || !d_count) return fail(c, KMC_ERR_ARG, "kmc_query_device: null device pointer");
    if ((((uintptr_t)d_key_hi | (uintptr_t)d_key_lo | (uintptr_t)d_count) & 7) != 0) return fail(c, KMC_ERR_ARG, "kmc_query_device: arrays must be 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return query_launch(c, (const u64*)d_key_hi, (const u64*)d_key_lo, n_keys, (u64*)d_count);
}

static int kmc_query_impl(kmc_ctx* c, const uint64_t* key_hi, const uint64_t* key_lo, uint64_t n_keys, uint64_t* count) {
    if (!c) return KMC_ERR_ARG;
    int rc = view_begin(c, "kmc_query");
    if (rc) return rc;
    if (!n_keys) return KMC_OK;
    if (!key_lo || !count) return fail(c, KMC_ERR_ARG, "kmc_query: null buffer");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t nb = (size_t)n_keys * sizeof(u64);
    if ((rc = ensure(c, c->q_klo, nb)) || (rc = ensure(c, c->q_cnt, nb))) return rc;
    if (key_hi && (rc = ensure(c, c->q_khi, nb))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->q_klo.p, key_lo, nb, hipMemcpyHostToDevice, c->stream));
    if (key_hi) HIPCHK(c, hipMemcpyAsync(c->q_khi.p, key_hi, nb, hipMemcpyHostToDevice, c->stream));
    rc = query_launch(c, key_hi ? (const u64*)c->q_khi.p : nullptr, (const u64*)c->q_klo.p, n_keys, (u64*)c->q_cnt.p);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(count, c->q_cnt.p, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KMC_OK;
}

// ---- a batch of reads for the kernels that walk it in chunks (kmc_chunks.hip.h): kmc_profile*, kmc_unitig_map* ----
// The launch that walks a batch whose results go to window STARTS: windows END up to k - 1 positions past the batch, and
// those (invalid) windows zero the last k - 1 slots.  A wave takes cpw chunks; grid workgroups of KMC_Q_THREADS.
struct ChunkGrid { u64 n_chunks, cpw, grid; };
static int chunk_grid(kmc_ctx* c, const char* what, u64 n_bases, int k, ChunkGrid* g) {
    g->n_chunks = (n_bases + (u64)k - 1 + KMC_CHUNK - 1) / KMC_CHUNK;
    const u64 want_waves = (u64)c->n_cu * 16;   // four waves on each SIMD
    g->cpw = std::min<u64>(64, std::max<u64>(1, (g->n_chunks + want_waves - 1) / want_waves));
    const u64 waves = (g->n_chunks + g->cpw - 1) / g->cpw;
    g->grid = (waves + KMC_Q_WAVES - 1) / KMC_Q_WAVES;
    if (g->grid > 0x7FFFFFFFull) return fail(c, KMC_ERR_ARG, "%s: batch too large for one call", what);
    return KMC_OK;
}

// a caller's device batch: d_bases is read 16 bytes at a time, d_offsets 8
static int check_device_batch(kmc_ctx* c, const char* what, const void* d_bases, const void* d_offsets) {
    if (!d_bases || !d_offsets) return fail(c, KMC_ERR_ARG, "%s: null device pointer", what);
    if (((uintptr_t)d_bases & 15) != 0) return fail(c, KMC_ERR_ARG, "%s: d_bases must be 16-byte aligned", what);
    if (((uintptr_t)d_offsets & 7) != 0) return fail(c, KMC_ERR_ARG, "%s: d_offsets must be 8-byte aligned", what);
    return KMC_OK;
}

// a host batch (n_reads > 0) checked and on its way into q_bases / q_offs; u32_reads: no read may have 2^32 bases or more
static int stage_batch(kmc_ctx* c, const char* what, const uint8_t* bases, const uint64_t* offsets, u64 n_reads, bool u32_reads, u64* n_bases) {
    if (!bases || !offsets) return fail(c, KMC_ERR_ARG, "%s: null buffer", what);
    if (offsets[0] != 0) return fail(c, KMC_ERR_ARG, "%s: offsets[0] must be 0", what);
    for (u64 i = 0; i < n_reads; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(c, KMC_ERR_ARG, "%s: offsets must be non-decreasing (read %llu)", what, (unsigned long long)i);
        if (u32_reads && offsets[i + 1] - offsets[i] >= (1ull << 32)) return fail(c, KMC_ERR_ARG, "%s: read %llu has 2^32 bases or more", what, (unsigned long long)i);
    }
    *n_bases = offsets[n_reads];
    HIPCHK(c, hipSetDevice(c->cfg.device));
    int rc;
    if ((rc = ensure(c, c->q_bases, *n_bases + 64)) || (rc = ensure(c, c->q_offs, (n_reads + 1) * sizeof(u64)))) return rc;
    if (*n_bases) HIPCHK(c, hipMemcpyAsync(c->q_bases.p, bases, *n_bases, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->q_offs.p, offsets, (n_reads + 1) * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    return KMC_OK;
}

// the profile launches (device arrays; either output may be null)
static int profile_launch(kmc_ctx* c, const uint8_t* d_bases, const u64* d_offsets, u64 n_reads, u64 n_bases, u64 min_count,
                          u32* d_win, u64* d_stats) {
    QView v;
    if (int rc = query_view(c, "kmc_profile", &v)) return rc;
    const int k = c->cfg.k;
    const u64 n_words = n_reads * KMC_PROFILE_WORDS;
    const u32 sgrid = (u32)((n_words + KMC_PROF_INIT_THREADS - 1) / KMC_PROF_INIT_THREADS);
    if (d_stats) hipLaunchKernelGGL(kmc_profile_init_kernel, dim3(sgrid), dim3(KMC_PROF_INIT_THREADS), 0, c->stream, (kmc_ull*)d_stats, n_reads);
    ChunkGrid g;
    if (int rc = chunk_grid(c, "kmc_profile", n_bases, k, &g)) return rc;
    if (g.n_chunks && (d_win || d_stats)) {
        const u64 thr = std::max<u64>(min_count, 1);
        with_kw_canon(c, [&](auto KW, auto CANON) {
            hipLaunchKernelGGL((kmc_profile_kernel<KW(), CANON()>), dim3((u32)g.grid), dim3(KMC_Q_THREADS), 0, c->stream, d_bases, n_bases,
                               d_offsets, n_reads, k, g.n_chunks, g.cpw, v, thr, d_win, (kmc_ull*)d_stats);
        });
    }
    if (d_stats) hipLaunchKernelGGL(kmc_profile_fix_kernel, dim3((u32)((n_reads + KMC_PROF_INIT_THREADS - 1) / KMC_PROF_INIT_THREADS)),
                                    dim3(KMC_PROF_INIT_THREADS), 0, c->stream, (kmc_ull*)d_stats, n_reads);
    HIPCHK(c, hipGetLastError());
    return KMC_OK;
}

static int kmc_profile_device_impl(kmc_ctx* c, const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
                                   uint64_t min_count, void* d_window_count, void* d_read_stats) {
    if (!c) return KMC_ERR_ARG;
    if (c->cfg.mode != KMC_MODE_CONTIG) return fail(c, KMC_ERR_ARG, "kmc_profile_device: contiguous k-mers only (not KMC_MODE_LR)");
    if (int rc = view_begin(c, "kmc_profile_device")) return rc;
    if (!n_reads) return KMC_OK;
    if (int rc = check_device_batch(c, "kmc_profile_device", d_bases, d_offsets)) return rc;
    if (((uintptr_t)d_read_stats & 7) != 0 || ((uintptr_t)d_window_count & 3) != 0)
        return fail(c, KMC_ERR_ARG, "kmc_profile_device: d_read_stats must be 8-byte, d_window_count 4-byte aligned");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return profile_launch(c, (const uint8_t*)d_bases, (const u64*)d_offsets, n_reads, n_bases, min_count, (u32*)d_window_count, (u64*)d_read_stats);
}

static int kmc_profile_impl(kmc_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t min_count,
                            uint32_t* window_count, uint64_t* read_stats) {
    if (!c) return KMC_ERR_ARG;
    if (c->cfg.mode != KMC_MODE_CONTIG) return fail(c, KMC_ERR_ARG, "kmc_profile: contiguous k-mers only (not KMC_MODE_LR)");
    int rc = view_begin(c, "kmc_profile");
    if (rc) return rc;
    if (!n_reads) return KMC_OK;
    u64 n_bases;
    if ((rc = stage_batch(c, "kmc_profile", bases, offsets, n_reads, false, &n_bases))) return rc;
    const size_t sb = (size_t)n_reads * KMC_PROFILE_WORDS * sizeof(u64), wb = (size_t)n_bases * sizeof(u32);
    if (window_count && n_bases && (rc = ensure(c, c->q_win, wb))) return rc;
    if (read_stats && (rc = ensure(c, c->q_stats, sb))) return rc;
    rc = profile_launch(c, (const uint8_t*)c->q_bases.p, (const u64*)c->q_offs.p, n_reads, n_bases, min_count,
                        window_count && n_bases ? (u32*)c->q_win.p : nullptr, read_stats ? (u64*)c->q_stats.p : nullptr);
    if (rc) return rc;
    if (window_count && n_bases) HIPCHK(c, hipMemcpyAsync(window_count, c->q_win.p, wb, hipMemcpyDeviceToHost, c->stream));
    if (read_stats) HIPCHK(c, hipMemcpyAsync(read_stats, c->q_stats.p, sb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KMC_OK;
}

// ---- two tables compared: summary and set operations over the sorted views of two contexts (kmc_setops.hip.h) ----
// a and b count the same kind of key on one device (the error is a's)
static int same_kind(kmc_ctx* a, const kmc_ctx* b, const char* what) {
    if (a->cfg.device != b->cfg.device) return fail(a, KMC_ERR_ARG, "%s: the contexts differ in device (%d / %d)", what, a->cfg.device, b->cfg.device);
    if (a->cfg.mode != b->cfg.mode) return fail(a, KMC_ERR_ARG, "%s: the contexts differ in mode (%d / %d)", what, a->cfg.mode, b->cfg.mode);
    if (a->klen != b->klen || a->KW != b->KW) return fail(a, KMC_ERR_ARG, "%s: the contexts differ in k (%d / %d)", what, a->klen, b->klen);
    if ((a->cfg.canonical != 0) != (b->cfg.canonical != 0))
        return fail(a, KMC_ERR_ARG, "%s: the contexts differ in canonical (%d / %d)", what, a->cfg.canonical, b->cfg.canonical);
    return KMC_OK;
}

// What every set-operation call checks first: arguments, that a and b count the same kind of key on one device, both views.
// b's view is only read, on a's stream: b is synchronised first where kmc_export_device would do so.
static int setop_begin(kmc_ctx* a, kmc_ctx* b, const char* what, int op, int count_mode, uint64_t min_a, uint64_t max_a,
                       uint64_t min_b, uint64_t max_b) {
    if (op < KMC_SETOP_INTERSECT || op > KMC_SETOP_SUBTRACT) return fail(a, KMC_ERR_ARG, "%s: unknown op %d", what, op);
    if (count_mode < KMC_COUNT_LEFT || count_mode > KMC_COUNT_DIFF) return fail(a, KMC_ERR_ARG, "%s: unknown count_mode %d", what, count_mode);
    if (max_a && min_a > max_a) return fail(a, KMC_ERR_ARG, "%s: min_a %llu > max_a %llu", what, (unsigned long long)min_a, (unsigned long long)max_a);
    if (max_b && min_b > max_b) return fail(a, KMC_ERR_ARG, "%s: min_b %llu > max_b %llu", what, (unsigned long long)min_b, (unsigned long long)max_b);
    int rc = same_kind(a, b, what);
    if (rc) return rc;
    rc = view_begin(a, what);
    if (rc) return rc;
    if (b != a) {
        if ((rc = view_begin(b, what)) || (rc = sync_view(b))) return rc;
    }
    if (a->n_sorted + b->n_sorted >= (1ull << 32))
        return fail(a, KMC_ERR_CAPACITY, "%s: the two views hold 2^32 keys or more together", what);
    HIPCHK(a, hipSetDevice(a->cfg.device));
    return KMC_OK;
}

static SoView so_view(const kmc_ctx* c, uint64_t min_c, uint64_t max_c) {
    return SoView{view_of(c), min_c, count_hi(max_c)};
}

// Partition + one pass over both views.  pass 0: the summary; pass 1: the summary, the emitted keys per tile and their
// scan (c_tpos).  h[0] = n_out (pass 1), h[1..8] = summary, h[9] = total_out.  Waits for the result.
static int setop_reduce(kmc_ctx* a, int pass, int op, int count_mode, const SoView& A, const SoView& B, u64* h) {
    memset(h, 0, (KMC_SO_WORDS + 1) * sizeof(u64));
    const u64 nm = A.n + B.n;
    if (!nm) return KMC_OK;
    if (!view_aligned16(A) || !view_aligned16(B)) return fail(a, KMC_ERR_HIP, "internal error: sorted view not 16-byte aligned");
    const u32 n_tiles = (u32)((nm + KMC_SO_TILE - 1) / KMC_SO_TILE);
    int rc;
    if ((rc = ensure(a, a->so_pa, ((size_t)n_tiles + 1) * sizeof(u32))) || (rc = ensure(a, a->so_pb, ((size_t)n_tiles + 1) * sizeof(u32))) ||
        (rc = compact_plan(a, n_tiles, KMC_SO_WORDS + 1)))   // [n_out | summary | total_out]
        return rc;
    kmc_ull* acc = (kmc_ull*)a->c_ctl.p + 1;
    u32 *pa = (u32*)a->so_pa.p, *pb = (u32*)a->so_pb.p, *tile = (u32*)a->c_tile.p;
    const u32 pgrid = (n_tiles + 1 + 255) / 256;
    const u32 grid = (u32)std::min<u64>(n_tiles, (u64)a->n_cu * 8);
    with_kw(a, [&](auto KW) {
        hipLaunchKernelGGL(kmc_setop_partition_kernel<KW()>, dim3(pgrid), dim3(256), 0, a->stream, A, B, n_tiles, pa, pb);
        if (pass == 0)
            hipLaunchKernelGGL((kmc_setop_join_kernel<KW(), 0>), dim3(grid), dim3(KMC_SO_THREADS), 0, a->stream, A, B, op, count_mode, n_tiles,
                               (const u32*)pa, (const u32*)pb, (u32*)nullptr, (const u32*)nullptr, acc, (u64*)nullptr, (u64*)nullptr, (u64*)nullptr);
        else
            hipLaunchKernelGGL((kmc_setop_join_kernel<KW(), 1>), dim3(grid), dim3(KMC_SO_THREADS), 0, a->stream, A, B, op, count_mode, n_tiles,
                               (const u32*)pa, (const u32*)pb, tile, (const u32*)nullptr, acc, (u64*)nullptr, (u64*)nullptr, (u64*)nullptr);
    });
    if (pass == 1) return compact_scan_and_read(a, n_tiles, h, KMC_SO_WORDS + 1);
    HIPCHK(a, hipGetLastError());   // the summary alone: nothing to scan
    HIPCHK(a, hipMemcpyAsync(h, a->c_ctl.p, (KMC_SO_WORDS + 1) * sizeof(u64), hipMemcpyDeviceToHost, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));
    return KMC_OK;
}

// scatter half (setop_reduce pass 1 ran first): the emitted entries into the set operation's result; finished when it returns
static int setop_scatter(kmc_ctx* a, int op, int count_mode, const SoView& A, const SoView& B, u64 n_out) {
    if (int rc = ensure_keys(a, a->so, n_out)) return rc;
    if (!n_out) return KMC_OK;
    const u32 n_tiles = (u32)((A.n + B.n + KMC_SO_TILE - 1) / KMC_SO_TILE);
    const u32 grid = (u32)std::min<u64>(n_tiles, (u64)a->n_cu * 8);
    with_kw(a, [&](auto KW) {
        hipLaunchKernelGGL((kmc_setop_join_kernel<KW(), 2>), dim3(grid), dim3(KMC_SO_THREADS), 0, a->stream, A, B, op, count_mode, n_tiles,
                           (const u32*)a->so_pa.p, (const u32*)a->so_pb.p, (u32*)nullptr, (const u32*)a->c_tpos.p, (kmc_ull*)nullptr,
                           (u64*)a->so.hi.p, (u64*)a->so.lo.p, (u64*)a->so.cnt.p);
    });
    HIPCHK(a, hipGetLastError());
    HIPCHK(a, hipStreamSynchronize(a->stream));
    return KMC_OK;
}

static int kmc_compare_impl(kmc_ctx* a, kmc_ctx* b, uint64_t min_a, uint64_t max_a, uint64_t min_b, uint64_t max_b, uint64_t* summary) {
    if (!a || !b) return a ? fail(a, KMC_ERR_ARG, "kmc_compare: null context") : KMC_ERR_ARG;
    if (!summary) return fail(a, KMC_ERR_ARG, "kmc_compare: null summary");
    u64 h[KMC_SO_WORDS + 1];
    int rc;
    if ((rc = setop_begin(a, b, "kmc_compare", KMC_SETOP_INTERSECT, KMC_COUNT_LEFT, min_a, max_a, min_b, max_b)) ||
        (rc = setop_reduce(a, 0, KMC_SETOP_INTERSECT, KMC_COUNT_LEFT, so_view(a, min_a, max_a), so_view(b, min_b, max_b), h))) return rc;
    memcpy(summary, h + 1, KMC_COMPARE_WORDS * sizeof(u64));
    return KMC_OK;
}

static int kmc_setop_device_impl(kmc_ctx* a, kmc_ctx* b, int op, int count_mode, uint64_t min_a, uint64_t max_a, uint64_t min_b,
                                 uint64_t max_b, const void** d_key_hi, const void** d_key_lo, const void** d_count, uint64_t* n_out,
                                 uint64_t* total_out, uint64_t* summary) {
    if (!a || !b) return a ? fail(a, KMC_ERR_ARG, "kmc_setop_device: null context") : KMC_ERR_ARG;
    int rc = setop_begin(a, b, "kmc_setop_device", op, count_mode, min_a, max_a, min_b, max_b);
    if (rc) return rc;
    const SoView A = so_view(a, min_a, max_a), B = so_view(b, min_b, max_b);
    u64 h[KMC_SO_WORDS + 1];
    if ((rc = setop_reduce(a, 1, op, count_mode, A, B, h)) || (rc = setop_scatter(a, op, count_mode, A, B, h[0]))) return rc;
    publish_keys(a, a->so, d_key_hi, d_key_lo, d_count);
    if (n_out) *n_out = h[0];
    if (total_out) *total_out = h[KMC_SO_WORDS];
    if (summary) memcpy(summary, h + 1, KMC_COMPARE_WORDS * sizeof(u64));
    return KMC_OK;
}

static int kmc_export_setop_impl(kmc_ctx* a, kmc_ctx* b, int op, int count_mode, uint64_t min_a, uint64_t max_a, uint64_t min_b,
                                 uint64_t max_b, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap, uint64_t* n_out) {
    if (n_out) *n_out = 0;
    if (!a || !b) return a ? fail(a, KMC_ERR_ARG, "kmc_export_setop: null context") : KMC_ERR_ARG;
    int rc = setop_begin(a, b, "kmc_export_setop", op, count_mode, min_a, max_a, min_b, max_b);
    if (rc) return rc;
    const SoView A = so_view(a, min_a, max_a), B = so_view(b, min_b, max_b);
    u64 h[KMC_SO_WORDS + 1];
    rc = setop_reduce(a, 1, op, count_mode, A, B, h);
    if (rc) return rc;
    const u64 n = h[0];
    if (n_out) *n_out = n;
    if (cap < n) return fail(a, KMC_ERR_ARG, "kmc_export_setop: capacity %llu < %llu result keys", (unsigned long long)cap, (unsigned long long)n);
    if (!n) return KMC_OK;
    if (!key_lo || !count) return fail(a, KMC_ERR_ARG, "null buffer");
    rc = setop_scatter(a, op, count_mode, A, B, n);
    if (rc) return rc;
    return copy_to_host(a, a->so.hi.p, a->so.lo.p, a->so.cnt.p, n, key_hi, key_lo, count);
}

// ---- the de Bruijn graph of the sorted view: neighbour masks, unitig ends, summary (kmc_graph.hip.h) ----
// What both calls check first; on success the view is resolved.
static int graph_begin(kmc_ctx* c, const char* what, uint64_t min_count, uint64_t max_count) {
    if (c->cfg.mode != KMC_MODE_CONTIG) return fail(c, KMC_ERR_ARG, "%s: contiguous k-mers only (not KMC_MODE_LR)", what);
    if (int rc = view_begin(c, what, min_count, max_count)) return rc;
    if (c->n_sorted >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: a view of 2^32 keys or more cannot be indexed", what);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return KMC_OK;
}

// adj of every view key into g_adj, the summary into h[KMC_GRAPH_WORDS]; finished when it returns (kmc_export_device's
// ordering contract).  Shares the prefix index with the query calls (query_view).
static int graph_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, u64* h) {
    memset(h, 0, KMC_GRAPH_WORDS * sizeof(u64));
    const u64 n = c->n_sorted;
    int rc;
    c->u_live = false;   // adj is rewritten from here on: a kept unitig result no longer has its work arrays
    c->m_idx_live = false;   // ... and the row index built from them (kmc_map.hip.h) goes with them
    if ((rc = ensure(c, c->g_adj, (size_t)std::max<u64>(n, 1) * sizeof(uint16_t))) || (rc = ensure(c, c->g_ctl, KMC_GRAPH_WORDS * sizeof(u64)))) return rc;
    if (!n) return KMC_OK;
    QView v;
    rc = query_view(c, what, &v);
    if (rc) return rc;
    kmc_ull* ctl = (kmc_ull*)c->g_ctl.p;
    HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_GRAPH_WORDS * sizeof(u64), c->stream));
    const u64 lo_c = std::max<u64>(min_count, 1), hi_c = count_hi(max_count);
    const u64 want = (n + KMC_G_THREADS - 1) / KMC_G_THREADS;
    const int k = c->klen;
    // as many workgroups as are resident at once (they walk the view with a grid stride), fewer for a small view
    with_kw_canon(c, [&](auto KW, auto CANON) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kmc_graph_kernel<KW(), CANON()>, KMC_G_THREADS, 0) != hipSuccess || per_cu < 1)
            per_cu = 4;
        const u32 grid = (u32)std::min<u64>(want, (u64)c->n_cu * (u64)per_cu);
        hipLaunchKernelGGL((kmc_graph_kernel<KW(), CANON()>), dim3(grid), dim3(KMC_G_THREADS), 0, c->stream, v, lo_c, hi_c, k,
                           (uint16_t*)c->g_adj.p, ctl);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h, ctl, KMC_GRAPH_WORDS * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KMC_OK;
}

static int kmc_graph_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void** d_adj, uint64_t* n_keys, uint64_t* summary) {
    if (!c) return KMC_ERR_ARG;
    u64 h[KMC_GRAPH_WORDS];
    int rc;
    if ((rc = graph_begin(c, "kmc_graph_device", min_count, max_count)) || (rc = graph_run(c, "kmc_graph_device", min_count, max_count, h))) return rc;
    if (d_adj) *d_adj = c->g_adj.p;
    if (n_keys) *n_keys = c->n_sorted;
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

static int kmc_graph_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, void* adj, uint64_t cap, uint64_t* n_keys, uint64_t* summary) {
    if (n_keys) *n_keys = 0;
    if (!c) return KMC_ERR_ARG;
    int rc = graph_begin(c, "kmc_graph", min_count, max_count);
    if (rc) return rc;
    const u64 n = c->n_sorted;
    if (n_keys) *n_keys = n;
    const bool sizing = !adj && !cap;   // the summary alone / how large adj must be
    if (!sizing && cap < n) return fail(c, KMC_ERR_ARG, "kmc_graph: capacity %llu < %llu keys of the view", (unsigned long long)cap, (unsigned long long)n);
    if (!sizing && n && !adj) return fail(c, KMC_ERR_ARG, "kmc_graph: null buffer");
    u64 h[KMC_GRAPH_WORDS];
    rc = graph_run(c, "kmc_graph", min_count, max_count, h);
    if (rc) return rc;
    if (adj && n) {
        HIPCHK(c, hipMemcpyAsync(adj, c->g_adj.p, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- the unitigs of that graph: sequences, offsets, abundances, flags, summary (kmc_unitig.hip.h) ----
// u_ctl: [0..7] the summary words ([0] while the call runs: keys the emit kernel could not place, always 0), [8] / [9] the totals of the two layout scans (unitigs, solid keys), then
// KMC_U_ROUND_SLOTS u32 counts of the ranking rounds
#define KMC_U_CTL_BYTES (10 * sizeof(u64) + KMC_U_ROUND_SLOTS * sizeof(u32))

// Phase times of one call on stderr when KMC_UNITIG_TRACE is set (tools/measure_unitigs.py reads them): event pairs on the
// ctx stream, read once at the end of the call.
struct UnitigTrace {
    static const int N = 8;
    bool on = getenv("KMC_UNITIG_TRACE") != nullptr;
    hipEvent_t ev[N] = {};
    int n_ev = 0;
    void mark(hipStream_t s) {
        if (on && n_ev < N && hipEventCreate(&ev[n_ev]) == hipSuccess) { (void)hipEventRecord(ev[n_ev], s); ++n_ev; }
    }
    void report(u64 n, u32 rounds, u32 cycle_states) {
        if (!on) return;
        static const char* const name[N - 1] = {"adj", "links", "ranking", "cycles", "layout", "emit", ""};
        fprintf(stderr, "kmc_unitigs: keys %llu rounds %u cycle_states %u", (unsigned long long)n, rounds, cycle_states);
        for (int i = 0; i + 1 < n_ev; ++i) {
            float ms = 0;
            if (hipEventSynchronize(ev[i + 1]) == hipSuccess && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess)
                fprintf(stderr, " %s_ms %.4f", name[i], ms);
        }
        fprintf(stderr, "\n");
    }
    ~UnitigTrace() { for (int i = 0; i < n_ev; ++i) (void)hipEventDestroy(ev[i]); }
};

// The arrays of a ranking: the unitigs' over the side states of the view rows (u_*), the contigs' over the node ends (ct_*)
struct RankBufs { u32* joined; u32* ptr[2]; u32* dist[2]; uint8_t* circ; u32* cnt; };   // (cnt: KMC_U_ROUND_SLOTS round counts)
static RankBufs unitig_bufs(kmc_ctx* c) {
    return RankBufs{(u32*)c->u_join.p, {(u32*)c->u_ptr[0].p, (u32*)c->u_ptr[1].p}, {(u32*)c->u_dist[0].p, (u32*)c->u_dist[1].p},
                    (uint8_t*)c->u_circ.p, (u32*)((u64*)c->u_ctl.p + 10)};
}

// Ranks the n2 side states along B.joined (kmc_unitig.hip.h): on return B.ptr[*cur] / B.dist[*cur] hold every path state's end
// and distance, *open the states on cycles, *rounds is raised by the rounds launched.  Waits for the result.
static int unitig_rank(kmc_ctx* c, const RankBufs& B, u64 n2, int* cur, u32* rounds, u32* open) {
    const u32* joined = B.joined;
    u32* const* ptr = B.ptr;
    u32* const* dist = B.dist;
    u32* cnt = B.cnt;
    const u32 grid = (u32)((n2 + KMC_U_THREADS - 1) / KMC_U_THREADS);
    HIPCHK(c, hipMemsetAsync(cnt, 0, KMC_U_ROUND_SLOTS * sizeof(u32), c->stream));
    hipLaunchKernelGGL(kmc_unitig_rank_init_kernel, dim3(grid), dim3(KMC_U_THREADS), 0, c->stream, joined, n2, ptr[0], dist[0], cnt);
    int max_rounds = 1;   // ceil(log2(n2)) + 1
    while ((1ull << (max_rounds - 1)) < n2) ++max_rounds;
    u32 h[KMC_U_ROUND_SLOTS] = {0};
    int t = 0, b = 0;
    bool done = false;
    while (!done && t < max_rounds) {
        const int batch = std::min(4, max_rounds - t);
        for (int i = 0; i < batch; ++i) {
            ++t;
            hipLaunchKernelGGL(kmc_unitig_rank_round_kernel, dim3(grid), dim3(KMC_U_THREADS), 0, c->stream, joined, n2, (const u32*)ptr[b],
                               (const u32*)dist[b], ptr[b ^ 1], dist[b ^ 1], cnt + t);
            b ^= 1;
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h, cnt, (size_t)(t + 1) * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int s = t - batch + 1; s <= t; ++s) done = done || h[s] == 0 || h[s] == h[s - 1];
    }
    *cur = b;
    *rounds += (u32)t;
    *open = h[t];
    return KMC_OK;
}

// The states the ranking left open lie on cycles (kmc_unitig.hip.h): every cycle is cut at side L of its smallest row, the
// row is marked in circ, and the ranking runs again.  Nothing to do when open is 0.
static int unitig_cut_cycles(kmc_ctx* c, const char* what, const RankBufs& B, u64 n, int* cur, u32* rounds, u32 open) {
    if (!open) return KMC_OK;
    const u64 n2 = 2 * n;
    const u32 grid_n = (u32)((n + KMC_U_THREADS - 1) / KMC_U_THREADS), grid_2n = (u32)((n2 + KMC_U_THREADS - 1) / KMC_U_THREADS);
    u32* const* ptr = B.ptr;
    u32* const* mrow = B.dist;
    hipLaunchKernelGGL(kmc_unitig_cycle_mark_kernel, dim3(grid_n), dim3(KMC_U_THREADS), 0, c->stream, (const u32*)B.joined,
                       (const u32*)ptr[*cur], n, B.circ);
    hipLaunchKernelGGL(kmc_unitig_minrow_init_kernel, dim3(grid_2n), dim3(KMC_U_THREADS), 0, c->stream, (const u32*)B.joined, n2, ptr[0], mrow[0]);
    int cover = 0, b = 0;   // 2^cover states of a cycle seen from every state: the longest cycle has at most `open`
    while ((1ull << cover) < open) ++cover;
    for (int i = 0; i < cover; ++i) {
        hipLaunchKernelGGL(kmc_unitig_minrow_round_kernel, dim3(grid_2n), dim3(KMC_U_THREADS), 0, c->stream, n2, (const u32*)ptr[b],
                           (const u32*)mrow[b], ptr[b ^ 1], mrow[b ^ 1]);
        b ^= 1;
    }
    hipLaunchKernelGGL(kmc_unitig_cycle_cut_kernel, dim3(grid_n), dim3(KMC_U_THREADS), 0, c->stream, (const u32*)mrow[b], n, B.joined, B.circ);
    HIPCHK(c, hipGetLastError());
    if (int rc = unitig_rank(c, B, n2, cur, rounds, &open)) return rc;
    if (open) return fail(c, KMC_ERR_HIP, "internal error: %s left %u side states on cycles after the cut", what, open);
    return KMC_OK;
}

// Everything on the device: the four arrays into the ctx's u_* buffers, the summary into h[KMC_UNITIG_WORDS]; finished
// when it returns (kmc_export_device's ordering contract).
static int unitig_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, u64* h) {
    memset(h, 0, KMC_UNITIG_WORDS * sizeof(u64));
    const u64 n = c->n_sorted, n2 = 2 * n;
    int rc;
    c->u_key.drop(); c->l_key.drop(); c->cc_key.drop(); c->bb_key.drop(); c->tx_key.drop(); c->ct_key.drop(); c->pr_key.drop();   // the result arrays are rewritten from here on (and the links of the old ones, their components, their bubbles, their transit counts and the pair records numbered by them go with them)
    if ((rc = ensure(c, c->u_offs, sizeof(u64))) || (rc = ensure(c, c->u_bases, 64)) || (rc = ensure(c, c->u_abund, sizeof(u64))) ||
        (rc = ensure(c, c->u_flags, 8)))
        return rc;
    if (!n) {
        HIPCHK(c, hipMemsetAsync(c->u_offs.p, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KMC_OK;
    }
    UnitigTrace tr;
    tr.mark(c->stream);
    u64 g[KMC_GRAPH_WORDS];
    if ((rc = graph_run(c, what, min_count, max_count, g))) return rc;
    tr.mark(c->stream);
    const size_t sb = (size_t)n2 * sizeof(u32);
    const size_t nsb = (size_t)((n + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK + 2) * sizeof(u32);
    if ((rc = ensure(c, c->u_link, sb)) || (rc = ensure(c, c->u_join, sb)) || (rc = ensure(c, c->u_ptr[0], sb)) ||
        (rc = ensure(c, c->u_ptr[1], sb)) || (rc = ensure(c, c->u_dist[0], sb)) || (rc = ensure(c, c->u_dist[1], sb)) ||
        (rc = ensure(c, c->u_circ, (size_t)n)) || (rc = ensure(c, c->u_ctl, KMC_U_CTL_BYTES)) || (rc = ensure(c, c->c_bsum, nsb)))
        return rc;
    QView v;
    if ((rc = query_view(c, what, &v))) return rc;
    const int k = c->klen, canon = c->cfg.canonical ? 1 : 0;
    const uint16_t* adj = (const uint16_t*)c->g_adj.p;
    u32 *link = (u32*)c->u_link.p, *joined = (u32*)c->u_join.p;
    uint8_t* circ = (uint8_t*)c->u_circ.p;
    kmc_ull* ctl = (kmc_ull*)c->u_ctl.p;
    const u32 grid_n = (u32)((n + KMC_U_THREADS - 1) / KMC_U_THREADS), grid_2n = (u32)((n2 + KMC_U_THREADS - 1) / KMC_U_THREADS);
    HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_U_CTL_BYTES, c->stream));
    HIPCHK(c, hipMemsetAsync(circ, 0, (size_t)n, c->stream));
    // links and joins
    with_kw_canon(c, [&](auto KW, auto CANON) {
        hipLaunchKernelGGL((kmc_unitig_link_kernel<KW(), CANON()>), dim3(grid_n), dim3(KMC_U_THREADS), 0, c->stream, v, k, adj, link);
    });
    hipLaunchKernelGGL(kmc_unitig_join_kernel, dim3(grid_2n), dim3(KMC_U_THREADS), 0, c->stream, (const u32*)link, n2, joined, ctl + 6);
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    // ranking; cycles, if there are any, are cut and the ranking runs again
    int cur = 0;
    u32 rounds = 0, open = 0, cycle_states = 0;
    const RankBufs B = unitig_bufs(c);
    if ((rc = unitig_rank(c, B, n2, &cur, &rounds, &open))) return rc;
    tr.mark(c->stream);
    cycle_states = open;
    if ((rc = unitig_cut_cycles(c, what, B, n, &cur, &rounds, open))) return rc;
    tr.mark(c->stream);
    // layout: first keys and their key counts (link is free now), their scans (joined is free now)
    const u32 *ptr = (const u32*)c->u_ptr[cur].p, *dist = (const u32*)c->u_dist[cur].p;
    u32 *is_first = link, *first_len = link + n, *uid_of = joined, *koff_of = joined + n;
    hipLaunchKernelGGL(kmc_unitig_place_kernel, dim3(grid_n), dim3(KMC_U_THREADS), 0, c->stream, n, adj, ptr, dist, canon, is_first, first_len);
    launch_exclusive_scan<0>(c->stream, is_first, (u32)n, (u32*)c->c_bsum.p, uid_of, (u32*)(ctl + 8));
    launch_exclusive_scan<0>(c->stream, first_len, (u32)n, (u32*)c->c_bsum.p, koff_of, (u32*)(ctl + 9));
    HIPCHK(c, hipGetLastError());
    u64 w[10];
    HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const u64 nu = w[8], nk = w[9], nb = nk + (u64)(k - 1) * nu;
    tr.mark(c->stream);
    // emit (d_bases is readable up to the next 16-byte boundary: the rule of kmc_add_batch_device)
    if ((rc = ensure(c, c->u_bases, (size_t)nb + 64)) || (rc = ensure(c, c->u_offs, (size_t)(nu + 1) * sizeof(u64))) ||
        (rc = ensure(c, c->u_abund, (size_t)std::max<u64>(nu, 1) * sizeof(u64))) || (rc = ensure(c, c->u_flags, (size_t)std::max<u64>(nu, 8))))
        return rc;
    HIPCHK(c, hipMemsetAsync(c->u_abund.p, 0, (size_t)std::max<u64>(nu, 1) * sizeof(u64), c->stream));
    with_kw(c, [&](auto KW) {
        hipLaunchKernelGGL(kmc_unitig_emit_kernel<KW()>, dim3((u32)grid_for(c, n, KMC_U_THREADS)), dim3(KMC_U_THREADS), 0, c->stream,
                           static_cast<const KView&>(v), k, canon, adj, ptr, dist, (const u32*)uid_of, (const u32*)koff_of, (const uint8_t*)circ,
                           nu, nb, (uint8_t*)c->u_bases.p, (u64*)c->u_offs.p, (kmc_ull*)c->u_abund.p, (uint8_t*)c->u_flags.p, ctl);
    });
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(w, ctl, KMC_UNITIG_WORDS * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tr.mark(c->stream);
    if (w[0]) return fail(c, KMC_ERR_HIP, "internal error: %s could not place %llu solid keys in the layout", what, (unsigned long long)w[0]);
    h[0] = nu; h[1] = nb; h[2] = nk; h[3] = w[3]; h[4] = w[4]; h[5] = w[5]; h[6] = w[6]; h[7] = w[7];
    c->u_cur = cur;      // what kmc_unitig_links reads: adj, u_ptr / u_dist[cur], uid_of in u_join
    c->u_live = true;
    tr.report(n, rounds, cycle_states);
    return KMC_OK;
}

static int unitig_begin(kmc_ctx* c, const char* what, uint64_t min_count, uint64_t max_count) {
    if (int rc = graph_begin(c, what, min_count, max_count)) return rc;
    if (c->n_sorted >= (1ull << 31)) return fail(c, KMC_ERR_CAPACITY, "%s: a view of 2^31 keys or more has more sides than a u32 numbers", what);
    return KMC_OK;
}

// the result arrays now hold the unitigs of this view and range (nothing but unitig_run writes them)
static void unitig_keep(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const u64* h) {
    c->u_key.keep(c->view_gen, min_count, max_count);
    memcpy(c->u_words, h, sizeof(c->u_words));
}

static int kmc_unitigs_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void** d_bases, const void** d_offsets,
                                   const void** d_abund, const void** d_flags, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* summary) {
    if (!c) return KMC_ERR_ARG;
    u64 h[KMC_UNITIG_WORDS];
    int rc;
    if ((rc = unitig_begin(c, "kmc_unitigs_device", min_count, max_count)) || (rc = unitig_run(c, "kmc_unitigs_device", min_count, max_count, h))) return rc;
    unitig_keep(c, min_count, max_count, h);
    if (d_bases) *d_bases = c->u_bases.p;
    if (d_offsets) *d_offsets = c->u_offs.p;
    if (d_abund) *d_abund = c->u_abund.p;
    if (d_flags) *d_flags = c->u_flags.p;
    if (n_unitigs) *n_unitigs = h[0];
    if (n_bases) *n_bases = h[1];
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

static int kmc_unitigs_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint8_t* bases, uint64_t cap_bases, uint64_t* offsets,
                            uint64_t* abund, uint8_t* flags, uint64_t cap_unitigs, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* summary) {
    if (n_unitigs) *n_unitigs = 0;
    if (n_bases) *n_bases = 0;
    if (!c) return KMC_ERR_ARG;
    u64 h[KMC_UNITIG_WORDS];
    int rc;
    if ((rc = unitig_begin(c, "kmc_unitigs", min_count, max_count))) return rc;
    if (c->u_key.holds(c->view_gen, min_count, max_count)) {
        memcpy(h, c->u_words, sizeof(h));   // the arrays of this view and range are still there: the call after a sizing call
    } else {
        if ((rc = unitig_run(c, "kmc_unitigs", min_count, max_count, h))) return rc;
        unitig_keep(c, min_count, max_count, h);
    }
    const u64 nu = h[0], nb = h[1];
    if (n_unitigs) *n_unitigs = nu;
    if (n_bases) *n_bases = nb;
    if (bases && cap_bases < nb)
        return fail(c, KMC_ERR_ARG, "kmc_unitigs: capacity %llu < %llu bases", (unsigned long long)cap_bases, (unsigned long long)nb);
    if ((offsets || abund || flags) && cap_unitigs < nu)
        return fail(c, KMC_ERR_ARG, "kmc_unitigs: capacity %llu < %llu unitigs", (unsigned long long)cap_unitigs, (unsigned long long)nu);
    if (bases && nb) HIPCHK(c, hipMemcpyAsync(bases, c->u_bases.p, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    if (offsets) HIPCHK(c, hipMemcpyAsync(offsets, c->u_offs.p, (size_t)(nu + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (abund && nu) HIPCHK(c, hipMemcpyAsync(abund, c->u_abund.p, (size_t)nu * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (flags && nu) HIPCHK(c, hipMemcpyAsync(flags, c->u_flags.p, (size_t)nu, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- the links between those unitigs: offsets per unitig end, target ends, summary (kmc_links.hip.h) ----
// The count pass keeps the targets it resolved in a scratch of 32 bytes per view row and the fill pass reads them
// (DESIGN.md has the numbers); KMC_LINKS_LOOKUP_TWICE in the environment makes the fill pass look them up again instead --
// a diagnostic for tools/measure_links.py, the result is the same.
template <bool FILL>
static void links_launch(kmc_ctx* c, const QView& v, bool scratch, u64 nu, u64 n_links) {
    const u64 want = (v.n + KMC_L_THREADS - 1) / KMC_L_THREADS;
    const int k = c->klen;
    with_kw_canon(c, [&](auto KW, auto CANON) {
        auto go = [&](auto SC) {
            auto kern = kmc_links_kernel<KW(), CANON(), FILL, SC()>;
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, KMC_L_THREADS, 0) != hipSuccess || per_cu < 1) per_cu = 4;
            const u32 grid = (u32)std::min<u64>(want, (u64)c->n_cu * (u64)per_cu);
            hipLaunchKernelGGL(kern, dim3(grid), dim3(KMC_L_THREADS), 0, c->stream, v, k, (const uint16_t*)c->g_adj.p,
                               (const u32*)c->u_ptr[c->u_cur].p, (const u32*)c->u_dist[c->u_cur].p, (const u32*)c->u_join.p, nu, n_links,
                               (u32*)c->l_tgt.p, (u32*)c->l_cnt.p, (const u32*)c->l_pos.p, (u32*)c->l_to.p, (kmc_ull*)c->l_ctl.p);
        };
        if (scratch) go(std::true_type{}); else go(std::false_type{});
    });
}

// The links of the unitigs the ctx holds (u_words, u_live) into l_offs / l_to, the summary into h[KMC_LINK_WORDS]; finished
// when it returns.
static int links_run(kmc_ctx* c, const char* what, u64* h) {
    memset(h, 0, KMC_LINK_WORDS * sizeof(u64));
    const u64 n = c->n_sorted, nu = c->u_words[0], ne = 2 * nu;
    int rc;
    c->l_key.drop(); c->cc_key.drop(); c->bb_key.drop(); c->tx_key.drop(); c->ct_key.drop();
    if ((rc = ensure(c, c->l_offs, (size_t)(ne + 1) * sizeof(u64))) || (rc = ensure(c, c->l_to, sizeof(u32)))) return rc;
    if (!nu) {   // an empty view, or one without a solid key
        HIPCHK(c, hipMemsetAsync(c->l_offs.p, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KMC_OK;
    }
    if (nu > n) return fail(c, KMC_ERR_HIP, "internal error: %s found %llu unitigs of %llu keys", what, (unsigned long long)nu, (unsigned long long)n);
    const bool scratch = getenv("KMC_LINKS_LOOKUP_TWICE") == nullptr;
    const size_t eb = (size_t)ne * sizeof(u32);
    if ((rc = ensure(c, c->l_cnt, eb)) || (rc = ensure(c, c->l_pos, eb)) || (rc = ensure(c, c->l_ctl, KMC_L_CTL_WORDS * sizeof(u64))) ||
        (rc = ensure(c, c->c_bsum, (size_t)((ne + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK + 2) * sizeof(u32))) ||
        (scratch && (rc = ensure(c, c->l_tgt, (size_t)n * 8 * sizeof(u32)))))
        return rc;
    QView v;
    if ((rc = query_view(c, what, &v))) return rc;
    kmc_ull* ctl = (kmc_ull*)c->l_ctl.p;
    HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_L_CTL_WORDS * sizeof(u64), c->stream));
    HIPCHK(c, hipMemsetAsync(c->l_cnt.p, 0, eb, c->stream));
    links_launch<false>(c, v, scratch, nu, 0);
    HIPCHK(c, hipGetLastError());
    u64 w[KMC_L_CTL_WORDS];
    HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[KMC_L_BAD]) return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays", what, (unsigned long long)w[KMC_L_BAD]);
    const u64 nl = w[1];
    if (nl >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: 2^32 link records or more", what);
    if ((rc = ensure(c, c->l_to, (size_t)std::max<u64>(nl, 1) * sizeof(u32)))) return rc;
    launch_exclusive_scan<0>(c->stream, c->l_cnt.p, (u32)ne, (u32*)c->c_bsum.p, (u32*)c->l_pos.p, (u32*)ctl);
    hipLaunchKernelGGL(kmc_links_offsets_kernel, dim3((u32)((nu + KMC_L_THREADS - 1) / KMC_L_THREADS)), dim3(KMC_L_THREADS), 0, c->stream,
                       (const u32*)c->l_cnt.p, (const u32*)c->l_pos.p, nu, nl, (u64*)c->l_offs.p, ctl);
    if (nl) links_launch<true>(c, v, scratch, nu, nl);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[KMC_L_BAD] || (w[0] & 0xFFFFFFFFull) != nl)
        return fail(c, KMC_ERR_HIP, "internal error: %s could not place its records (%llu outside, %llu scanned of %llu)", what,
                    (unsigned long long)w[KMC_L_BAD], (unsigned long long)(w[0] & 0xFFFFFFFFull), (unsigned long long)nl);
    h[0] = nu; h[1] = nl;
    for (int i = 2; i < KMC_LINK_WORDS; ++i) h[i] = w[i];
    return KMC_OK;
}

// What both calls do once their arguments are in order: the kept links (host form only), or the links pass behind the
// kept unitigs of this view and range if their work arrays are still theirs, or behind a unitig_run of its own.
static int links_result(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, bool may_reuse, u64* h) {
    if (may_reuse && c->l_key.holds(c->view_gen, min_count, max_count)) {
        memcpy(h, c->l_words, sizeof(c->l_words));
        return KMC_OK;
    }
    int rc;
    const bool kept = c->u_live && c->u_key.holds(c->view_gen, min_count, max_count);
    if (!kept) {
        u64 t[KMC_UNITIG_WORDS];
        if ((rc = unitig_run(c, what, min_count, max_count, t))) return rc;
        unitig_keep(c, min_count, max_count, t);
    }
    UnitigTrace tr;
    tr.mark(c->stream);
    if ((rc = links_run(c, what, h))) return rc;
    tr.mark(c->stream);
    if (tr.on && tr.n_ev == 2) {
        float ms = 0;
        if (hipEventSynchronize(tr.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, tr.ev[0], tr.ev[1]) == hipSuccess)
            fprintf(stderr, "kmc_unitig_links: keys %llu unitigs %llu records %llu unitigs_reused %d links_ms %.4f\n",
                    (unsigned long long)c->n_sorted, (unsigned long long)h[0], (unsigned long long)h[1], kept ? 1 : 0, ms);
    }
    c->l_key.keep(c->view_gen, min_count, max_count);
    memcpy(c->l_words, h, sizeof(c->l_words));
    return KMC_OK;
}

static int kmc_unitig_links_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void** d_link_offsets,
                                        const void** d_link_to, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* summary) {
    if (!c) return KMC_ERR_ARG;
    u64 h[KMC_LINK_WORDS];
    int rc;
    if ((rc = unitig_begin(c, "kmc_unitig_links_device", min_count, max_count)) ||
        (rc = links_result(c, "kmc_unitig_links_device", min_count, max_count, false, h))) return rc;
    if (d_link_offsets) *d_link_offsets = c->l_offs.p;
    if (d_link_to) *d_link_to = c->l_to.p;
    if (n_unitigs) *n_unitigs = h[0];
    if (n_links) *n_links = h[1];
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

static int kmc_unitig_links_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t* link_offsets, uint64_t cap_ends,
                                 uint32_t* link_to, uint64_t cap_links, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* summary) {
    if (n_unitigs) *n_unitigs = 0;
    if (n_links) *n_links = 0;
    if (!c) return KMC_ERR_ARG;
    u64 h[KMC_LINK_WORDS];
    int rc;
    if ((rc = unitig_begin(c, "kmc_unitig_links", min_count, max_count)) ||
        (rc = links_result(c, "kmc_unitig_links", min_count, max_count, true, h))) return rc;
    const u64 ne = 2 * h[0], nl = h[1];
    if (n_unitigs) *n_unitigs = h[0];
    if (n_links) *n_links = nl;
    if (link_offsets && cap_ends < ne)
        return fail(c, KMC_ERR_ARG, "kmc_unitig_links: capacity %llu < %llu unitig ends", (unsigned long long)cap_ends, (unsigned long long)ne);
    if (link_to && cap_links < nl)
        return fail(c, KMC_ERR_ARG, "kmc_unitig_links: capacity %llu < %llu records", (unsigned long long)cap_links, (unsigned long long)nl);
    if (link_offsets) HIPCHK(c, hipMemcpyAsync(link_offsets, c->l_offs.p, (size_t)(ne + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (link_to && nl) HIPCHK(c, hipMemcpyAsync(link_to, c->l_to.p, (size_t)nl * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- reads threaded through those unitigs: place words, segments, per-read and per-unitig totals (kmc_map.hip.h) ----
// KMC_MAP_NO_INDEX in the environment makes the place kernel gather adj, the ranking and uid_of per window instead of the
// row index -- a diagnostic for tools/measure_map.py, the result is the same.
template <int PASS>
static void map_segs_launch(kmc_ctx* c, const MapBatch& b, u64 n_segs, u64 nu) {
    const u32 grid = (u32)std::min<u64>(b.n_tiles, (u64)c->n_cu * 8);
    hipLaunchKernelGGL(kmc_map_segs_kernel<PASS>, dim3(grid), dim3(KMC_M_THREADS), 0, c->stream, b, (u32*)c->c_tile.p, (const u32*)c->c_tpos.p,
                       n_segs, nu, (u32*)c->m_tail.p, (uint4*)c->m_segs.p, (u64*)c->m_soffs.p, (u32*)c->m_stats.p, (kmc_ull*)c->m_support.p,
                       (kmc_ull*)c->c_ctl.p);
}

// The batch (device arrays) laid on the unitigs of this view and range -- those the ctx holds if their work arrays are
// still theirs, otherwise computed and kept -- into the m_* buffers; h[KMC_MAP_WORDS] the summary.  Finished when it returns.
static int map_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, const uint8_t* d_bases, const u64* d_offsets, u64 n_reads,
                   u64 n_bases, u64* h, u64* n_segs, u64* n_unitigs) {
    memset(h, 0, KMC_MAP_WORDS * sizeof(u64));
    *n_segs = *n_unitigs = 0;
    int rc;
    const bool kept = c->u_live && c->u_key.holds(c->view_gen, min_count, max_count);
    if (!kept) {
        u64 t[KMC_UNITIG_WORDS];
        if ((rc = unitig_run(c, what, min_count, max_count, t))) return rc;
        unitig_keep(c, min_count, max_count, t);
    }
    const u64 n = c->n_sorted, nu = c->u_words[0];
    *n_unitigs = nu;
    if (nu > n) return fail(c, KMC_ERR_HIP, "internal error: %s holds %llu unitigs of %llu keys", what, (unsigned long long)nu, (unsigned long long)n);
    const int k = c->klen;
    const u64 n_tiles = (n_bases + 1 + KMC_M_TILE - 1) / KMC_M_TILE;
    if (n_tiles >= (1ull << 31)) return fail(c, KMC_ERR_ARG, "%s: batch too large for one call", what);
    ChunkGrid g;
    if ((rc = chunk_grid(c, what, n_bases, k, &g))) return rc;
    const size_t stb = (size_t)std::max<u64>(n_reads, 1) * KMC_MAP_READ_WORDS * sizeof(u32), spb = (size_t)std::max<u64>(nu, 1) * sizeof(u64);
    const size_t bitb = (size_t)std::max<u64>(g.n_chunks, 1) * 64 * sizeof(uint16_t);
    if ((rc = ensure(c, c->m_soffs, (size_t)(n_reads + 1) * sizeof(u64))) || (rc = ensure(c, c->m_stats, stb)) || (rc = ensure(c, c->m_support, spb)) ||
        (rc = ensure(c, c->m_segs, 16)) || (rc = ensure(c, c->m_tail, 4)) || (rc = ensure(c, c->m_idx, (size_t)std::max<u64>(n, 1) * sizeof(u64))) ||
        (rc = ensure(c, c->m_place, (size_t)std::max<u64>(n_bases, 1) * sizeof(u64))) || (rc = ensure(c, c->m_sbits, bitb)) ||
        (rc = ensure(c, c->m_vbits, bitb)) || (rc = compact_plan(c, n_tiles, KMC_M_CTL_WORDS)))
        return rc;
    HIPCHK(c, hipMemsetAsync(c->m_stats.p, 0, stb, c->stream));
    HIPCHK(c, hipMemsetAsync(c->m_support.p, 0, spb, c->stream));
    if (!n_reads) {
        HIPCHK(c, hipMemsetAsync(c->m_soffs.p, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KMC_OK;
    }
    QView v;
    if ((rc = query_view(c, what, &v))) return rc;
    kmc_ull* ctl = (kmc_ull*)c->c_ctl.p;
    const int canon = c->cfg.canonical ? 1 : 0;
    const bool use_index = getenv("KMC_MAP_NO_INDEX") == nullptr;
    UnitigTrace tr;
    tr.mark(c->stream);
    if (n && use_index && !c->m_idx_live) {   // once per unitig result: graph_run, which every unitig_run goes through, clears m_idx_live
        hipLaunchKernelGGL(kmc_map_index_kernel, dim3((u32)((n + KMC_M_THREADS - 1) / KMC_M_THREADS)), dim3(KMC_M_THREADS), 0, c->stream, n,
                           (const uint16_t*)c->g_adj.p, (const u32*)c->u_ptr[c->u_cur].p, (const u32*)c->u_dist[c->u_cur].p, (const u32*)c->u_join.p,
                           canon, nu, (u64*)c->m_idx.p, ctl);
        HIPCHK(c, hipGetLastError());
        c->m_idx_live = true;
    }
    tr.mark(c->stream);
    {
        MapSrc src;
        src.idx = (const u64*)c->m_idx.p; src.adj = (const uint16_t*)c->g_adj.p;
        src.ptr = (const u32*)c->u_ptr[c->u_cur].p; src.dist = (const u32*)c->u_dist[c->u_cur].p; src.uid_of = (const u32*)c->u_join.p;
        src.n_unitigs = nu;
        if (g.n_chunks) with_kw_canon(c, [&](auto KW, auto CANON) {
            auto go = [&](auto INDEX) {
                hipLaunchKernelGGL((kmc_map_place_kernel<KW(), CANON(), INDEX()>), dim3((u32)g.grid), dim3(KMC_Q_THREADS), 0, c->stream, d_bases, n_bases,
                                   d_offsets, n_reads, k, g.n_chunks, g.cpw, v, src, (u64*)c->m_place.p, (uint16_t*)c->m_sbits.p, (uint16_t*)c->m_vbits.p, ctl);
            };
            if (use_index) go(std::true_type{}); else go(std::false_type{});
        });
        HIPCHK(c, hipGetLastError());
    }
    tr.mark(c->stream);
    MapBatch b;
    b.place = (const u64*)c->m_place.p; b.start_bits = (const uint16_t*)c->m_sbits.p; b.valid_bits = (const uint16_t*)c->m_vbits.p;
    b.offsets = d_offsets; b.n_reads = n_reads; b.n_bases = n_bases; b.n_tiles = n_tiles; b.k = k;
    map_segs_launch<0>(c, b, 0, nu);
    u64 w[KMC_M_CTL_WORDS];
    if ((rc = compact_scan_and_read(c, n_tiles, w, KMC_M_CTL_WORDS))) return rc;
    if (w[KMC_M_BAD]) return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays", what, (unsigned long long)w[KMC_M_BAD]);
    const u64 ns = w[KMC_M_HEADS];
    if (ns >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: 2^32 segments or more", what);
    if ((w[0] & 0xFFFFFFFFull) != ns)
        return fail(c, KMC_ERR_HIP, "internal error: %s scanned %llu of %llu segments", what, (unsigned long long)(w[0] & 0xFFFFFFFFull), (unsigned long long)ns);
    if ((rc = ensure(c, c->m_segs, (size_t)std::max<u64>(ns, 1) * 4 * sizeof(u32))) || (rc = ensure(c, c->m_tail, (size_t)std::max<u64>(ns, 1) * sizeof(u32))))
        return rc;
    map_segs_launch<1>(c, b, ns, nu);
    hipLaunchKernelGGL(kmc_map_reads_kernel, dim3((u32)grid_for(c, n_reads, KMC_M_THREADS)), dim3(KMC_M_THREADS), 0, c->stream,
                       (const u32*)c->m_stats.p, d_offsets, n_reads, ctl);
    if (ns) map_segs_launch<2>(c, b, ns, nu);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tr.mark(c->stream);
    if (w[KMC_M_BAD]) return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays", what, (unsigned long long)w[KMC_M_BAD]);
    if (w[KMC_M_LONG]) return fail(c, KMC_ERR_ARG, "%s: %llu reads of 2^32 bases or more", what, (unsigned long long)w[KMC_M_LONG]);
    h[0] = n_reads; h[1] = w[KMC_M_VALID]; h[2] = w[KMC_M_PLACED]; h[3] = ns; h[4] = w[KMC_M_CROSS];
    h[5] = w[KMC_M_FULL]; h[6] = w[KMC_M_EMPTY]; h[7] = w[KMC_M_MOST];
    *n_segs = ns;
    if (tr.on && tr.n_ev == 4) {
        float ms[3] = {0, 0, 0};
        bool ok = hipEventSynchronize(tr.ev[3]) == hipSuccess;
        for (int i = 0; ok && i < 3; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_unitig_map: keys %llu unitigs %llu reads %llu windows %llu placed %llu segments %llu unitigs_reused %d "
                    "index_ms %.4f place_ms %.4f segs_ms %.4f\n", (unsigned long long)n, (unsigned long long)nu, (unsigned long long)n_reads,
                    (unsigned long long)h[1], (unsigned long long)h[2], (unsigned long long)ns, kept ? 1 : 0, ms[0], ms[1], ms[2]);
    }
    return KMC_OK;
}

static int map_begin(kmc_ctx* c, const char* what, uint64_t min_count, uint64_t max_count) { return unitig_begin(c, what, min_count, max_count); }

static int kmc_unitig_map_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void* d_bases, const void* d_offsets,
                                      uint64_t n_reads, uint64_t n_bases, const void** d_place, const void** d_read_stats,
                                      const void** d_seg_offsets, const void** d_segs, const void** d_support, uint64_t* n_segs,
                                      uint64_t* n_unitigs, uint64_t* summary) {
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_unitig_map_device";
    int rc;
    if ((rc = map_begin(c, what, min_count, max_count))) return rc;
    if (n_reads && (rc = check_device_batch(c, what, d_bases, d_offsets))) return rc;
    u64 h[KMC_MAP_WORDS], ns = 0, nu = 0;
    if ((rc = map_run(c, what, min_count, max_count, (const uint8_t*)d_bases, (const u64*)d_offsets, n_reads, n_reads ? n_bases : 0, h, &ns, &nu)))
        return rc;
    if (d_place) *d_place = c->m_place.p;
    if (d_read_stats) *d_read_stats = c->m_stats.p;
    if (d_seg_offsets) *d_seg_offsets = c->m_soffs.p;
    if (d_segs) *d_segs = c->m_segs.p;
    if (d_support) *d_support = c->m_support.p;
    if (n_segs) *n_segs = ns;
    if (n_unitigs) *n_unitigs = nu;
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

static int kmc_unitig_map_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                               uint64_t* place, uint32_t* read_stats, uint64_t* seg_offsets, uint32_t* segs, uint64_t cap_segs,
                               uint64_t* support, uint64_t cap_unitigs, uint64_t* n_segs, uint64_t* n_unitigs, uint64_t* summary) {
    if (n_segs) *n_segs = 0;
    if (n_unitigs) *n_unitigs = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_unitig_map";
    int rc;
    if ((rc = map_begin(c, what, min_count, max_count))) return rc;
    u64 n_bases = 0;
    if (n_reads && (rc = stage_batch(c, what, bases, offsets, n_reads, true, &n_bases))) return rc;
    u64 h[KMC_MAP_WORDS], ns = 0, nu = 0;
    if ((rc = map_run(c, what, min_count, max_count, (const uint8_t*)c->q_bases.p, (const u64*)c->q_offs.p, n_reads, n_bases, h, &ns, &nu))) return rc;
    if (n_segs) *n_segs = ns;
    if (n_unitigs) *n_unitigs = nu;
    if (segs && cap_segs < ns) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu segments", what, (unsigned long long)cap_segs, (unsigned long long)ns);
    if (support && cap_unitigs < nu) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu unitigs", what, (unsigned long long)cap_unitigs, (unsigned long long)nu);
    if (place && n_bases) HIPCHK(c, hipMemcpyAsync(place, c->m_place.p, (size_t)n_bases * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (read_stats && n_reads) HIPCHK(c, hipMemcpyAsync(read_stats, c->m_stats.p, (size_t)n_reads * KMC_MAP_READ_WORDS * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    if (seg_offsets) HIPCHK(c, hipMemcpyAsync(seg_offsets, c->m_soffs.p, (size_t)(n_reads + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (segs && ns) HIPCHK(c, hipMemcpyAsync(segs, c->m_segs.p, (size_t)ns * 4 * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    if (support && nu) HIPCHK(c, hipMemcpyAsync(support, c->m_support.p, (size_t)nu * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- read walks counted per link record and per unitig: support, transit matrices, verdicts (kmc_transits.hip.h) ----
// KMC_TRANSITS_PLAIN in the environment makes every lane of the transit kernel add its own 1 instead of combining equal
// targets per wave -- a diagnostic for tools/measure_transits.py, the result is the same.
static int transits_flags(kmc_ctx* c, const char* what, uint32_t flags) {
    if (flags & ~(uint32_t)KMC_TRANSIT_ACCUMULATE) return fail(c, KMC_ERR_ARG, "%s: unknown flag bits 0x%x", what, flags & ~(uint32_t)KMC_TRANSIT_ACCUMULATE);
    return KMC_OK;
}

// The batch (device arrays) walked through the unitigs and links of this view and range -- those the ctx holds under
// bubbles_run's condition, otherwise computed and kept -- into the tx_* buffers, the summary into tx_words; finished when it
// returns.  Links first, then the map passes, then the transit passes: a links call that computes may not run behind the map
// passes whose ids it would renumber.  It shares the block sums of a scan (c_bsum) with the other passes and, through
// map_run, the map buffers; it writes nothing else of theirs.
static int transits_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, u64 min_reads, bool accumulate, const uint8_t* d_bases,
                        const u64* d_offsets, u64 n_reads, u64 n_bases) {
    int rc;
    u64 lw[KMC_LINK_WORDS];
    const bool held = c->u_live && c->u_key.holds(c->view_gen, min_count, max_count);
    const bool links_reused = held && c->l_key.holds(c->view_gen, min_count, max_count);
    if (accumulate && !(links_reused && c->tx_key.holds(c->view_gen, min_count, max_count)))
        return fail(c, KMC_ERR_STATE, "%s: KMC_TRANSIT_ACCUMULATE, and the ctx holds no transits of this view and range to add to", what);
    c->ct_key.drop();   // the counts a held contig result was made from change
    if ((rc = links_result(c, what, min_count, max_count, held, lw))) return rc;
    const u64 n = c->n_sorted, nu = lw[0], nl = lw[1];
    if (nu > n || c->u_words[0] != nu)
        return fail(c, KMC_ERR_HIP, "internal error: %s holds %llu unitigs, its links %llu", what, (unsigned long long)c->u_words[0], (unsigned long long)nu);
    TransitGraph g;
    g.link_offsets = (const u64*)c->l_offs.p; g.link_to = (const u32*)c->l_to.p; g.n_unitigs = nu; g.n_links = nl;
    const u32 grid_u = (u32)((nu + KMC_T_THREADS - 1) / KMC_T_THREADS);
    if ((rc = ensure(c, c->tx_ctl, KMC_T_CTL_WORDS * sizeof(u64)))) return rc;
    kmc_ull* ctl = (kmc_ull*)c->tx_ctl.p;
    u64 w[KMC_T_CTL_WORDS] = {0};
    HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_T_CTL_WORDS * sizeof(u64), c->stream));
    if (!accumulate) {
        // the layout: it depends on the links alone
        c->tx_key.drop();
        const size_t lb = (size_t)std::max<u64>(nl, 1) * sizeof(u64);
        if ((rc = ensure(c, c->tx_sup, lb)) || (rc = ensure(c, c->tx_offs, (size_t)(nu + 1) * sizeof(u64))) ||
            (rc = ensure(c, c->tx_verdict, (size_t)std::max<u64>(nu, 1))) || (rc = ensure(c, c->tx_count, sizeof(u64))))
            return rc;
        u64 n_slots = 0;
        if (nu) {
            const size_t ub = (size_t)nu * sizeof(u32);
            if ((rc = ensure(c, c->tx_cnt, ub)) || (rc = ensure(c, c->tx_pos, ub)) ||
                (rc = ensure(c, c->c_bsum, (size_t)((nu + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK + 2) * sizeof(u32))))
                return rc;
            hipLaunchKernelGGL(kmc_transit_layout_kernel, dim3(grid_u), dim3(KMC_T_THREADS), 0, c->stream, g, (u32*)c->tx_cnt.p, ctl);
            launch_exclusive_scan<0>(c->stream, c->tx_cnt.p, (u32)nu, (u32*)c->c_bsum.p, (u32*)c->tx_pos.p, (u32*)(ctl + KMC_T_SCAN));
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (w[KMC_T_BAD]) return fail(c, KMC_ERR_HIP, "internal error: %s met %llu ends whose records lie outside their array", what, (unsigned long long)w[KMC_T_BAD]);
            n_slots = w[KMC_T_SLOTS];
            if (n_slots >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: 2^32 transit slots or more", what);
            if ((w[KMC_T_SCAN] & 0xFFFFFFFFull) != n_slots)
                return fail(c, KMC_ERR_HIP, "internal error: %s scanned %llu of %llu slots", what, (unsigned long long)(w[KMC_T_SCAN] & 0xFFFFFFFFull), (unsigned long long)n_slots);
            if ((rc = ensure(c, c->tx_count, (size_t)std::max<u64>(n_slots, 1) * sizeof(u64)))) return rc;
            hipLaunchKernelGGL(kmc_transit_offsets_kernel, dim3(grid_u), dim3(KMC_T_THREADS), 0, c->stream, (const u32*)c->tx_pos.p, nu, n_slots, (u64*)c->tx_offs.p);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_T_CTL_WORDS * sizeof(u64), c->stream));
        } else {
            HIPCHK(c, hipMemsetAsync(c->tx_offs.p, 0, sizeof(u64), c->stream));
        }
        HIPCHK(c, hipMemsetAsync(c->tx_sup.p, 0, lb, c->stream));
        HIPCHK(c, hipMemsetAsync(c->tx_count.p, 0, (size_t)std::max<u64>(n_slots, 1) * sizeof(u64), c->stream));
        c->tx_slots = n_slots;
        memset(c->tx_words, 0, sizeof(c->tx_words));
    }
    const u64 n_slots = c->tx_slots;
    UnitigTrace tr;
    tr.mark(c->stream);
    // the map passes: they find the unitigs held, so they renumber nothing (tx_ctl is not theirs)
    u64 mh[KMC_MAP_WORDS] = {0}, ns = 0, mu = nu;
    if (n_reads && nu) {
        if ((rc = map_run(c, what, min_count, max_count, d_bases, d_offsets, n_reads, n_bases, mh, &ns, &mu))) return rc;
        if (mu != nu || !c->l_key.holds(c->view_gen, min_count, max_count))
            return fail(c, KMC_ERR_HIP, "internal error: %s mapped onto %llu unitigs, its links know %llu", what, (unsigned long long)mu, (unsigned long long)nu);
    }
    tr.mark(c->stream);
    if (ns) {
        if ((rc = ensure(c, c->tx_first, (size_t)ns))) return rc;
        HIPCHK(c, hipMemsetAsync(c->tx_first.p, 0, (size_t)ns, c->stream));
        hipLaunchKernelGGL(kmc_transit_first_kernel, dim3((u32)((n_reads + KMC_T_THREADS - 1) / KMC_T_THREADS)), dim3(KMC_T_THREADS), 0, c->stream,
                           (const u64*)c->m_soffs.p, n_reads, ns, (uint8_t*)c->tx_first.p, ctl);
        const u32 grid = (u32)grid_for(c, ns, KMC_T_THREADS);
        auto go = [&](auto COMBINE) {
            hipLaunchKernelGGL(kmc_transit_kernel<COMBINE()>, dim3(grid), dim3(KMC_T_THREADS), 0, c->stream, g, (const uint4*)c->m_segs.p,
                               (const uint8_t*)c->tx_first.p, ns, (const u64*)c->tx_offs.p, n_slots, (kmc_ull*)c->tx_sup.p, (kmc_ull*)c->tx_count.p, ctl);
        };
        if (getenv("KMC_TRANSITS_PLAIN") == nullptr) go(std::true_type{}); else go(std::false_type{});
        HIPCHK(c, hipGetLastError());
    }
    tr.mark(c->stream);
    const u64 nx = std::max(nu, nl);
    if (nx) {
        hipLaunchKernelGGL(kmc_transit_verdict_kernel, dim3((u32)((nx + KMC_T_THREADS - 1) / KMC_T_THREADS)), dim3(KMC_T_THREADS), 0, c->stream, g,
                           (const u64*)c->tx_offs.p, n_slots, (const kmc_ull*)c->tx_sup.p, (const kmc_ull*)c->tx_count.p, std::max<u64>(min_reads, 1),
                           (uint8_t*)c->tx_verdict.p, ctl);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tr.mark(c->stream);
    if (w[KMC_T_BAD] || w[KMC_T_CROSS] != mh[4]) {
        c->tx_key.drop();   // the arrays may hold a part of this batch
        return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays (%llu crossings, the map pass %llu)", what,
                    (unsigned long long)w[KMC_T_BAD], (unsigned long long)w[KMC_T_CROSS], (unsigned long long)mh[4]);
    }
    u64* s = c->tx_words;
    s[0] += w[KMC_T_CROSS]; s[1] += w[KMC_T_ORPHAN]; s[3] += w[KMC_T_STORED]; s[4] += w[KMC_T_DROPPED];
    s[2] = w[KMC_T_ZERO]; s[5] = w[KMC_T_REPEAT]; s[6] = w[KMC_T_RESOLVED]; s[7] = w[KMC_T_AMBIG];
    c->tx_key.keep(c->view_gen, min_count, max_count);
    if (tr.on && tr.n_ev == 4) {
        float ms[3] = {0, 0, 0};
        bool ok = hipEventSynchronize(tr.ev[3]) == hipSuccess;
        for (int i = 0; ok && i < 3; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_unitig_transits: unitigs %llu records %llu reads %llu segments %llu crossings %llu transits %llu links_reused %d "
                    "map_ms %.4f transit_ms %.4f verdict_ms %.4f\n", (unsigned long long)nu, (unsigned long long)nl, (unsigned long long)n_reads,
                    (unsigned long long)ns, (unsigned long long)w[KMC_T_CROSS], (unsigned long long)w[KMC_T_STORED], links_reused ? 1 : 0, ms[0], ms[1], ms[2]);
    }
    return KMC_OK;
}

static int kmc_unitig_transits_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint32_t flags,
                                           const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
                                           const void** d_link_support, const void** d_transit_offsets, const void** d_transit_count,
                                           const void** d_verdict, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* n_slots, uint64_t* summary) {
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_unitig_transits_device";
    int rc;
    if ((rc = map_begin(c, what, min_count, max_count)) || (rc = transits_flags(c, what, flags))) return rc;
    if (n_reads && (rc = check_device_batch(c, what, d_bases, d_offsets))) return rc;
    if ((rc = transits_run(c, what, min_count, max_count, min_reads, (flags & KMC_TRANSIT_ACCUMULATE) != 0, (const uint8_t*)d_bases,
                           (const u64*)d_offsets, n_reads, n_reads ? n_bases : 0)))
        return rc;
    if (d_link_support) *d_link_support = c->tx_sup.p;
    if (d_transit_offsets) *d_transit_offsets = c->tx_offs.p;
    if (d_transit_count) *d_transit_count = c->tx_count.p;
    if (d_verdict) *d_verdict = c->tx_verdict.p;
    if (n_unitigs) *n_unitigs = c->l_words[0];
    if (n_links) *n_links = c->l_words[1];
    if (n_slots) *n_slots = c->tx_slots;
    if (summary) memcpy(summary, c->tx_words, sizeof(c->tx_words));
    return KMC_OK;
}

static int kmc_unitig_transits_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint32_t flags, const uint8_t* bases,
                                    const uint64_t* offsets, uint64_t n_reads, uint64_t* link_support, uint64_t cap_links,
                                    uint64_t* transit_offsets, uint64_t cap_unitigs, uint64_t* transit_count, uint64_t cap_slots, uint8_t* verdict,
                                    uint64_t* n_unitigs, uint64_t* n_links, uint64_t* n_slots, uint64_t* summary) {
    if (n_unitigs) *n_unitigs = 0;
    if (n_links) *n_links = 0;
    if (n_slots) *n_slots = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_unitig_transits";
    int rc;
    if ((rc = map_begin(c, what, min_count, max_count)) || (rc = transits_flags(c, what, flags))) return rc;
    u64 n_bases = 0;
    if (n_reads && (rc = stage_batch(c, what, bases, offsets, n_reads, true, &n_bases))) return rc;
    if ((rc = transits_run(c, what, min_count, max_count, min_reads, (flags & KMC_TRANSIT_ACCUMULATE) != 0, (const uint8_t*)c->q_bases.p,
                           (const u64*)c->q_offs.p, n_reads, n_bases)))
        return rc;
    const u64 nu = c->l_words[0], nl = c->l_words[1], nsl = c->tx_slots;
    if (n_unitigs) *n_unitigs = nu;
    if (n_links) *n_links = nl;
    if (n_slots) *n_slots = nsl;
    if (link_support && cap_links < nl) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu records", what, (unsigned long long)cap_links, (unsigned long long)nl);
    if ((transit_offsets || verdict) && cap_unitigs < nu) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu unitigs", what, (unsigned long long)cap_unitigs, (unsigned long long)nu);
    if (transit_count && cap_slots < nsl) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu slots", what, (unsigned long long)cap_slots, (unsigned long long)nsl);
    if (link_support && nl) HIPCHK(c, hipMemcpyAsync(link_support, c->tx_sup.p, (size_t)nl * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (transit_offsets) HIPCHK(c, hipMemcpyAsync(transit_offsets, c->tx_offs.p, (size_t)(nu + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (transit_count && nsl) HIPCHK(c, hipMemcpyAsync(transit_count, c->tx_count.p, (size_t)nsl * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (verdict && nu) HIPCHK(c, hipMemcpyAsync(verdict, c->tx_verdict.p, (size_t)nu, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, c->tx_words, sizeof(c->tx_words));
    return KMC_OK;
}

// ---- pair evidence: the ends the mates of a pair connect, the bases between them, insert sizes (kmc_pairs.hip.h) ----
// KMC_PAIRS_PLAIN in the environment makes every lane of the reduce kernel issue its own atomics instead of combining per
// workgroup in LDS -- a diagnostic for tools/measure_pairs.py, the result is the same.
static int pairs_args(kmc_ctx* c, const char* what, uint64_t n_bins, uint32_t flags, uint64_t n_reads) {
    if (flags & ~(uint32_t)KMC_PAIR_ACCUMULATE) return fail(c, KMC_ERR_ARG, "%s: unknown flag bits 0x%x", what, flags & ~(uint32_t)KMC_PAIR_ACCUMULATE);
    if (n_bins < 2 || n_bins > (1ull << 20)) return fail(c, KMC_ERR_ARG, "%s: n_bins %llu outside 2..2^20", what, (unsigned long long)n_bins);
    if (n_reads & 1) return fail(c, KMC_ERR_ARG, "%s: %llu reads are no whole number of pairs", what, (unsigned long long)n_reads);
    return KMC_OK;
}

// The pairs of the batch (device arrays) laid on the unitigs of this view and range -- those the ctx holds under map_run's
// condition, otherwise computed and kept -- into the pr_* buffers, the summary into pr_words; finished when it returns.  The
// map passes first, then anchor, class, sort, records, reduce.  Through map_run it shares the map buffers; through
// sort_keys_to_run the sort's scratch and the run pool; it writes nothing else that is not its own.
static int pairs_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, u64 n_bins, bool accumulate, const uint8_t* d_bases,
                     const u64* d_offsets, u64 n_reads, u64 n_bases) {
    int rc;
    const bool kept = c->u_live && c->u_key.holds(c->view_gen, min_count, max_count);
    if (accumulate && !(kept && c->pr_key.holds(c->view_gen, min_count, max_count) && c->pr_bins == n_bins))
        return fail(c, KMC_ERR_STATE, "%s: KMC_PAIR_ACCUMULATE, and the ctx holds no pairs of this view, range and n_bins to add to", what);
    const size_t hb = (size_t)n_bins * sizeof(u64);
    if ((rc = ensure(c, c->pr_ctl, KMC_P_CTL_WORDS * sizeof(u64))) || (rc = ensure(c, c->pr_hist, hb))) return rc;
    if (!accumulate) {
        c->pr_key.drop();
        c->pr_records = 0;
        memset(c->pr_words, 0, sizeof(c->pr_words));
        HIPCHK(c, hipMemsetAsync(c->pr_hist.p, 0, hb, c->stream));
    }
    UnitigTrace tr;
    tr.mark(c->stream);
    // the map passes (with no read they still see to the unitigs)
    u64 mh[KMC_MAP_WORDS] = {0}, ns = 0, nu = 0;
    if ((rc = map_run(c, what, min_count, max_count, d_bases, d_offsets, n_reads, n_bases, mh, &ns, &nu))) return rc;
    if (accumulate && !c->pr_key.holds(c->view_gen, min_count, max_count))
        return fail(c, KMC_ERR_HIP, "internal error: %s computed the unitigs under a held pairs result", what);
    if (nu > (1ull << 30)) return fail(c, KMC_ERR_CAPACITY, "%s: more than 2^30 unitigs", what);
    if (accumulate && n_reads == 0) return KMC_OK;   // nothing to add: the held result as it stands, its pointers included
    int end_bits = 5;   // (ten key bits at least: what the sort's first level takes)
    while ((1ull << end_bits) < 2 * nu) ++end_bits;
    tr.mark(c->stream);
    const u64 n_pairs = n_reads / 2, n_old = accumulate ? c->pr_records : 0, n_sort = n_pairs + n_old;
    if (n_sort >= (1ull << 32) - (1ull << 24)) return fail(c, KMC_ERR_CAPACITY, "%s: 2^32 pairs and held records or more", what);
    const int cur = c->pr_cur, nxt = cur ^ 1;
    kmc_ull* ctl = (kmc_ull*)c->pr_ctl.p;
    u64 w[KMC_P_CTL_WORDS] = {0};
    HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_P_CTL_WORDS * sizeof(u64), c->stream));
    const size_t sb = (size_t)std::max<u64>(n_sort, 1) * sizeof(u64), pb = (size_t)std::max<u64>(n_pairs, 1);
    if ((rc = ensure(c, c->pr_anchor, (size_t)std::max<u64>(n_reads, 1) * 16)) || (rc = ensure(c, c->pr_class, pb)) ||
        (rc = ensure(c, c->pr_ends, pb * 2 * sizeof(u32))) || (rc = ensure(c, c->pr_value, pb * sizeof(u64))) ||
        (rc = ensure(c, c->pr_sk[0], sb)) || (rc = ensure(c, c->pr_sk[1], sb)) || (rc = ensure(c, c->pr_sw[0], sb)) || (rc = ensure(c, c->pr_sw[1], sb)))
        return rc;
    // from here on the held result is in the making (the pair pass adds to the held histogram): an error leaves none
    auto give_up = [&](int code) { c->pr_key.drop(); return code; };
    auto hip_ok = [&](hipError_t e, const char* step) { return e == hipSuccess ? KMC_OK : give_up(fail(c, KMC_ERR_HIP, "%s: %s: %s", what, step, hipGetErrorString(e))); };
    // KMC_PAIRS_GRID (diagnostic, read per call): at most this many workgroups for the pair and reduce passes, so that a test
    // sends a small batch through many rounds of one workgroup
    u64 max_grid = ~0ull;
    if (const char* e = getenv("KMC_PAIRS_GRID")) max_grid = std::max<u64>(1, strtoull(e, nullptr, 10));
    if (n_pairs) {
        hipLaunchKernelGGL(kmc_pair_anchor_kernel, dim3((u32)((n_reads + KMC_P_THREADS - 1) / KMC_P_THREADS)), dim3(KMC_P_THREADS), 0, c->stream,
                           (const u64*)c->m_soffs.p, (const uint4*)c->m_segs.p, n_reads, ns, (const u64*)c->u_offs.p, nu, c->klen, (uint4*)c->pr_anchor.p, ctl);
        hipLaunchKernelGGL(kmc_pair_class_kernel, dim3((u32)std::min<u64>(grid_for(c, n_pairs, KMC_P_THREADS), max_grid)), dim3(KMC_P_THREADS), 0, c->stream,
                           (const uint4*)c->pr_anchor.p, n_pairs, (const u64*)c->u_offs.p, nu, end_bits, n_bins, (uint8_t*)c->pr_class.p, (u32*)c->pr_ends.p,
                           (u64*)c->pr_value.p, (u64*)c->pr_sk[0].p, (u64*)c->pr_sw[0].p, (kmc_ull*)c->pr_hist.p, ctl);
        if ((rc = hip_ok(hipGetLastError(), "the pair passes"))) return rc;
    }
    if (n_old) {   // the held records: keys with their counts as weights
        if ((rc = hip_ok(hipMemcpyAsync((u64*)c->pr_sk[0].p + n_pairs, c->pr_rkey[cur].p, (size_t)n_old * sizeof(u64), hipMemcpyDeviceToDevice, c->stream), "the held keys")) ||
            (rc = hip_ok(hipMemcpyAsync((u64*)c->pr_sw[0].p + n_pairs, c->pr_rcount[cur].p, (size_t)n_old * sizeof(u64), hipMemcpyDeviceToDevice, c->stream), "the held counts")))
            return rc;
    }
    tr.mark(c->stream);
    kmc_ctx::Run run;
    if (n_sort) {
        u64* const klo[2] = {(u64*)c->pr_sk[0].p, (u64*)c->pr_sk[1].p};
        u64* const kwt[2] = {(u64*)c->pr_sw[0].p, (u64*)c->pr_sw[1].p};
        if ((rc = sort_keys_to_run(c, klo, kwt, n_sort, 2u * (unsigned)end_bits, &run))) return give_up(rc);
    }
    const u64 n_rec = run.n;
    tr.mark(c->stream);
    const size_t rb = (size_t)std::max<u64>(n_rec, 1) * sizeof(u64);
    if ((rc = ensure(c, c->pr_rkey[nxt], rb)) || (rc = ensure(c, c->pr_rends[nxt], rb)) || (rc = ensure(c, c->pr_rcount[nxt], rb)) ||
        (rc = ensure(c, c->pr_rsum[nxt], rb)) || (rc = ensure(c, c->pr_rmin[nxt], rb)) || (rc = ensure(c, c->pr_rmax[nxt], rb))) {
        recycle_run(c, &run);
        return give_up(rc);
    }
    if (n_rec) {
        hipLaunchKernelGGL(kmc_pair_records_kernel, dim3((u32)((n_rec + KMC_P_THREADS - 1) / KMC_P_THREADS)), dim3(KMC_P_THREADS), 0, c->stream,
                           (const u64*)run.lo, (const u64*)run.cnt, n_rec, end_bits, 2 * nu, (u64*)c->pr_rkey[nxt].p, (u32*)c->pr_rends[nxt].p,
                           (u64*)c->pr_rcount[nxt].p, (u64*)c->pr_rsum[nxt].p, (u64*)c->pr_rmin[nxt].p, (u64*)c->pr_rmax[nxt].p, ctl);
        auto go = [&](auto TABLE) {
            hipLaunchKernelGGL(kmc_pair_reduce_kernel<TABLE()>, dim3((u32)std::min<u64>(grid_for(c, n_sort, KMC_P_THREADS), max_grid)), dim3(KMC_P_THREADS), 0, c->stream,
                               (const uint8_t*)c->pr_class.p, (const u32*)c->pr_ends.p, (const u64*)c->pr_value.p, n_pairs, (const u64*)c->pr_rkey[cur].p,
                               (const u64*)c->pr_rsum[cur].p, (const u64*)c->pr_rmin[cur].p, (const u64*)c->pr_rmax[cur].p, n_old, end_bits,
                               (const u64*)c->pr_rkey[nxt].p, n_rec, (kmc_ull*)c->pr_rsum[nxt].p, (kmc_ull*)c->pr_rmin[nxt].p, (kmc_ull*)c->pr_rmax[nxt].p, ctl);
        };
        if (getenv("KMC_PAIRS_PLAIN") == nullptr) go(std::true_type{}); else go(std::false_type{});
    }
    hipLaunchKernelGGL(kmc_pair_hist_sum_kernel, dim3((u32)((n_bins + KMC_P_THREADS - 1) / KMC_P_THREADS)), dim3(KMC_P_THREADS), 0, c->stream,
                       (const kmc_ull*)c->pr_hist.p, n_bins, ctl);
    const hipError_t le = hipGetLastError();
    recycle_run(c, &run);   // (stream order: the records kernel is queued before anything can reuse it)
    if (le != hipSuccess) return give_up(fail(c, KMC_ERR_HIP, "%s: %s", what, hipGetErrorString(le)));
    if (hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return give_up(fail(c, KMC_ERR_HIP, "%s: the pair passes failed", what));
    tr.mark(c->stream);
    if (w[KMC_P_BAD] || w[KMC_P_MISS])
        return give_up(fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays and %llu keys without a record", what,
                            (unsigned long long)w[KMC_P_BAD], (unsigned long long)w[KMC_P_MISS]));
    u64* s = c->pr_words;
    s[0] += n_pairs;
    for (int j = 0; j < 5; ++j) s[1 + j] += w[KMC_P_CLASS + j];
    s[6] = n_rec; s[7] += w[KMC_P_SUMF];
    // the identities of include/kmc.h
    if (s[0] != s[1] + s[2] + s[3] + s[4] + s[5] || (n_rec ? w[KMC_P_RCOUNT] : 0) != s[2] || w[KMC_P_HIST] != s[3] || n_rec > s[2] || n_rec >= (1ull << 32))
        return give_up(fail(c, n_rec >= (1ull << 32) ? KMC_ERR_CAPACITY : KMC_ERR_HIP,
                            "%s: %llu records; internal error unless 2^32 or more: %llu pairs in classes %llu %llu %llu %llu %llu, counts %llu, histogram %llu", what,
                            (unsigned long long)n_rec, (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[2], (unsigned long long)s[3],
                            (unsigned long long)s[4], (unsigned long long)s[5], (unsigned long long)w[KMC_P_RCOUNT], (unsigned long long)w[KMC_P_HIST]));
    c->pr_cur = nxt;
    c->pr_records = n_rec;
    c->pr_bins = n_bins;
    c->pr_key.keep(c->view_gen, min_count, max_count);
    if (tr.on && tr.n_ev == 5) {
        float ms[4] = {0, 0, 0, 0};
        bool ok = hipEventSynchronize(tr.ev[4]) == hipSuccess;
        for (int i = 0; ok && i < 4; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_unitig_pairs: unitigs %llu pairs %llu span %llu proper %llu records %llu unitigs_reused %d "
                    "map_ms %.4f anchor_ms %.4f sort_ms %.4f reduce_ms %.4f\n", (unsigned long long)nu, (unsigned long long)n_pairs,
                    (unsigned long long)w[KMC_P_CLASS + KMC_PAIR_SPAN], (unsigned long long)w[KMC_P_CLASS + KMC_PAIR_PROPER], (unsigned long long)n_rec,
                    kept ? 1 : 0, ms[0], ms[1], ms[2], ms[3]);
    }
    return KMC_OK;
}

static int kmc_unitig_pairs_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t n_bins, uint32_t flags, const void* d_bases,
                                        const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void** d_pair_class,
                                        const void** d_pair_ends, const void** d_pair_value, const void** d_rec_ends, const void** d_rec_count,
                                        const void** d_rec_sum, const void** d_rec_min, const void** d_rec_max, const void** d_insert_hist,
                                        uint64_t* n_pairs, uint64_t* n_records, uint64_t* summary) {
    if (n_pairs) *n_pairs = 0;
    if (n_records) *n_records = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_unitig_pairs_device";
    int rc;
    if ((rc = map_begin(c, what, min_count, max_count)) || (rc = pairs_args(c, what, n_bins, flags, n_reads))) return rc;
    if (n_reads && (rc = check_device_batch(c, what, d_bases, d_offsets))) return rc;
    if ((rc = pairs_run(c, what, min_count, max_count, n_bins, (flags & KMC_PAIR_ACCUMULATE) != 0, (const uint8_t*)d_bases, (const u64*)d_offsets,
                        n_reads, n_reads ? n_bases : 0)))
        return rc;
    const int cur = c->pr_cur;
    if (d_pair_class) *d_pair_class = c->pr_class.p;
    if (d_pair_ends) *d_pair_ends = c->pr_ends.p;
    if (d_pair_value) *d_pair_value = c->pr_value.p;
    if (d_rec_ends) *d_rec_ends = c->pr_rends[cur].p;
    if (d_rec_count) *d_rec_count = c->pr_rcount[cur].p;
    if (d_rec_sum) *d_rec_sum = c->pr_rsum[cur].p;
    if (d_rec_min) *d_rec_min = c->pr_rmin[cur].p;
    if (d_rec_max) *d_rec_max = c->pr_rmax[cur].p;
    if (d_insert_hist) *d_insert_hist = c->pr_hist.p;
    if (n_pairs) *n_pairs = n_reads / 2;
    if (n_records) *n_records = c->pr_records;
    if (summary) memcpy(summary, c->pr_words, sizeof(c->pr_words));
    return KMC_OK;
}

static int kmc_unitig_pairs_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t n_bins, uint32_t flags, const uint8_t* bases,
                                 const uint64_t* offsets, uint64_t n_reads, uint8_t* pair_class, uint32_t* pair_ends, uint64_t* pair_value,
                                 uint64_t cap_pairs, uint32_t* rec_ends, uint64_t* rec_count, uint64_t* rec_sum, uint64_t* rec_min, uint64_t* rec_max,
                                 uint64_t cap_records, uint64_t* insert_hist, uint64_t cap_bins, uint64_t* n_pairs, uint64_t* n_records,
                                 uint64_t* summary) {
    if (n_pairs) *n_pairs = 0;
    if (n_records) *n_records = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_unitig_pairs";
    int rc;
    if ((rc = map_begin(c, what, min_count, max_count)) || (rc = pairs_args(c, what, n_bins, flags, n_reads))) return rc;
    u64 n_bases = 0;
    if (n_reads && (rc = stage_batch(c, what, bases, offsets, n_reads, true, &n_bases))) return rc;
    if ((rc = pairs_run(c, what, min_count, max_count, n_bins, (flags & KMC_PAIR_ACCUMULATE) != 0, (const uint8_t*)c->q_bases.p,
                        (const u64*)c->q_offs.p, n_reads, n_bases)))
        return rc;
    const u64 np = n_reads / 2, nr = c->pr_records;
    const int cur = c->pr_cur;
    if (n_pairs) *n_pairs = np;
    if (n_records) *n_records = nr;
    if ((pair_class || pair_ends || pair_value) && cap_pairs < np)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu pairs", what, (unsigned long long)cap_pairs, (unsigned long long)np);
    if ((rec_ends || rec_count || rec_sum || rec_min || rec_max) && cap_records < nr)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu records", what, (unsigned long long)cap_records, (unsigned long long)nr);
    if (insert_hist && cap_bins < n_bins) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu bins", what, (unsigned long long)cap_bins, (unsigned long long)n_bins);
    auto down = [&](void* dst, const DevBuf& src, size_t bytes) {
        return dst && bytes ? hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    HIPCHK(c, down(pair_class, c->pr_class, (size_t)np));
    HIPCHK(c, down(pair_ends, c->pr_ends, (size_t)np * 2 * sizeof(u32)));
    HIPCHK(c, down(pair_value, c->pr_value, (size_t)np * sizeof(u64)));
    HIPCHK(c, down(rec_ends, c->pr_rends[cur], (size_t)nr * 2 * sizeof(u32)));
    HIPCHK(c, down(rec_count, c->pr_rcount[cur], (size_t)nr * sizeof(u64)));
    HIPCHK(c, down(rec_sum, c->pr_rsum[cur], (size_t)nr * sizeof(u64)));
    HIPCHK(c, down(rec_min, c->pr_rmin[cur], (size_t)nr * sizeof(u64)));
    HIPCHK(c, down(rec_max, c->pr_rmax[cur], (size_t)nr * sizeof(u64)));
    HIPCHK(c, down(insert_hist, c->pr_hist, (size_t)n_bins * sizeof(u64)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, c->pr_words, sizeof(c->pr_words));
    return KMC_OK;
}

// ---- the counted walks acted on: resolved repeats duplicated, unsupported links ignored, contigs spelled (kmc_contigs.hip.h) ----
// What both calls check first.  The call computes nothing it was not given: the unitigs, the links and a transits result of
// this view and range must be held (the result keys, not the work arrays: a kmc_graph* call in between does not matter).
static int contigs_begin(kmc_ctx* c, const char* what, uint64_t min_count, uint64_t max_count) {
    if (int rc = unitig_begin(c, what, min_count, max_count)) return rc;
    const char* missing = !c->u_key.holds(c->view_gen, min_count, max_count)    ? "unitigs (kmc_unitigs*)"
                          : !c->l_key.holds(c->view_gen, min_count, max_count)  ? "links (kmc_unitig_links*)"
                          : !c->tx_key.holds(c->view_gen, min_count, max_count) ? "transits (kmc_unitig_transits*)"
                                                                                : nullptr;
    if (missing) return fail(c, KMC_ERR_STATE, "%s: the ctx holds no %s of this view and range", what, missing);
    return KMC_OK;
}

static bool contigs_kept(const kmc_ctx* c, u64 min_count, u64 max_count, u64 min_reads, u64 min_support) {
    return c->ct_key.holds(c->view_gen, min_count, max_count) && c->ct_reads == min_reads && c->ct_support == min_support;
}

// The contigs of the held unitigs, links and transit counts into the ct_* buffers, the summary into h[KMC_CONTIG_WORDS];
// finished when it returns.  It reads u_bases / u_offs / u_abund, l_offs / l_to, tx_sup / tx_offs / tx_count and writes
// nothing but its own buffers and the block sums of a scan (c_bsum).
static int contigs_run(kmc_ctx* c, const char* what, u64 min_reads, u64 min_support, u64* h) {
    memset(h, 0, KMC_CONTIG_WORDS * sizeof(u64));
    const u64 nu = c->u_words[0], u_nb = c->u_words[1], nl = c->l_words[1], n_slots = c->tx_slots;
    const int k = c->klen;
    int rc;
    c->ct_key.drop();
    if ((rc = ensure(c, c->ct_offs, sizeof(u64))) || (rc = ensure(c, c->ct_poffs, sizeof(u64))) || (rc = ensure(c, c->ct_bases, 64)) ||
        (rc = ensure(c, c->ct_path, sizeof(u32))) || (rc = ensure(c, c->ct_abund, sizeof(u64))) || (rc = ensure(c, c->ct_flags, 8)))
        return rc;
    if (!nu) {   // an empty view, or one without a solid key
        HIPCHK(c, hipMemsetAsync(c->ct_offs.p, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipMemsetAsync(c->ct_poffs.p, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KMC_OK;
    }
    if (c->l_words[0] != nu) return fail(c, KMC_ERR_HIP, "internal error: %s holds %llu unitigs, its links %llu", what, (unsigned long long)nu, (unsigned long long)c->l_words[0]);
    UnitigTrace tr;
    tr.mark(c->stream);
    TransitGraph g;
    g.link_offsets = (const u64*)c->l_offs.p; g.link_to = (const u32*)c->l_to.p; g.n_unitigs = nu; g.n_links = nl;
    const auto blocks = [](u64 n) { return dim3((u32)((n + KMC_CT_THREADS - 1) / KMC_CT_THREADS)); };
    const auto bsum_bytes = [](u64 n) { return (size_t)((n + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK + 2) * sizeof(u32); };
    // nodes: copies and sigma per unitig, node_offsets
    if ((rc = ensure(c, c->ct_copies, (size_t)nu * sizeof(u32))) || (rc = ensure(c, c->ct_sigma, (size_t)nu)) ||
        (rc = ensure(c, c->ct_pos, (size_t)nu * sizeof(u32))) || (rc = ensure(c, c->ct_ctl, KMC_CT_CTL_BYTES)) || (rc = ensure(c, c->c_bsum, bsum_bytes(nu))))
        return rc;
    kmc_ull* ctl = (kmc_ull*)c->ct_ctl.p;
    u64 w[KMC_CT_CTL_WORDS];
    const auto read_ctl = [&]() -> int {
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (w[KMC_CT_BAD]) return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays", what, (unsigned long long)w[KMC_CT_BAD]);
        return KMC_OK;
    };
    HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_CT_CTL_BYTES, c->stream));
    const u32* copies = (const u32*)c->ct_copies.p;
    const uint8_t* sigma = (const uint8_t*)c->ct_sigma.p;
    const u32* node_offsets = (const u32*)c->ct_pos.p;
    hipLaunchKernelGGL(kmc_contig_nodes_kernel, blocks(nu), dim3(KMC_CT_THREADS), 0, c->stream, g, (const u64*)c->tx_offs.p, n_slots,
                       (const kmc_ull*)c->tx_sup.p, (const kmc_ull*)c->tx_count.p, std::max<u64>(min_reads, 1), min_support, (u32*)c->ct_copies.p,
                       (uint8_t*)c->ct_sigma.p, ctl);
    launch_exclusive_scan<0>(c->stream, copies, (u32)nu, (u32*)c->c_bsum.p, (u32*)c->ct_pos.p, (u32*)(ctl + KMC_CT_SCAN_N));
    if ((rc = read_ctl())) return rc;
    const u64 nn = w[KMC_CT_NODES], n2 = 2 * nn;
    if (nn >= (1ull << 31)) return fail(c, KMC_ERR_CAPACITY, "%s: 2^31 nodes or more have more ends than a u32 numbers", what);
    if ((w[KMC_CT_SCAN_N] & 0xFFFFFFFFull) != nn || nn < nu)
        return fail(c, KMC_ERR_HIP, "internal error: %s scanned %llu of %llu nodes", what, (unsigned long long)(w[KMC_CT_SCAN_N] & 0xFFFFFFFFull), (unsigned long long)nn);
    // choice and join over the 2 * nn node ends
    const size_t sb = (size_t)n2 * sizeof(u32);
    if ((rc = ensure(c, c->ct_owner, (size_t)nn * sizeof(u32))) || (rc = ensure(c, c->ct_link, sb)) || (rc = ensure(c, c->ct_join, sb)) ||
        (rc = ensure(c, c->ct_ptr[0], sb)) || (rc = ensure(c, c->ct_ptr[1], sb)) || (rc = ensure(c, c->ct_dist[0], sb)) ||
        (rc = ensure(c, c->ct_dist[1], sb)) || (rc = ensure(c, c->ct_circ, (size_t)nn)) || (rc = ensure(c, c->c_bsum, bsum_bytes(nn))))
        return rc;
    const u32* owner = (const u32*)c->ct_owner.p;
    u32 *link = (u32*)c->ct_link.p, *joined = (u32*)c->ct_join.p;
    HIPCHK(c, hipMemsetAsync(c->ct_circ.p, 0, (size_t)nn, c->stream));
    hipLaunchKernelGGL(kmc_contig_owner_kernel, blocks(nu), dim3(KMC_CT_THREADS), 0, c->stream, copies, node_offsets, nu, nn, (u32*)c->ct_owner.p, ctl);
    hipLaunchKernelGGL(kmc_contig_choice_kernel, blocks(n2), dim3(KMC_CT_THREADS), 0, c->stream, g, (const kmc_ull*)c->tx_sup.p, min_support, copies, sigma,
                       node_offsets, owner, nn, link, ctl);
    hipLaunchKernelGGL(kmc_unitig_join_kernel, blocks(n2), dim3(KMC_U_THREADS), 0, c->stream, (const u32*)link, n2, joined, ctl + KMC_CT_UNJOINED);
    if ((rc = read_ctl())) return rc;   // (before the ranking follows the choices)
    tr.mark(c->stream);
    // ranking; cycles, if there are any, are cut at the START end of their smallest node and the ranking runs again
    const RankBufs B{joined, {(u32*)c->ct_ptr[0].p, (u32*)c->ct_ptr[1].p}, {(u32*)c->ct_dist[0].p, (u32*)c->ct_dist[1].p}, (uint8_t*)c->ct_circ.p,
                     (u32*)(ctl + KMC_CT_CTL_WORDS)};
    int cur = 0;
    u32 rounds = 0, open = 0;
    if ((rc = unitig_rank(c, B, n2, &cur, &rounds, &open)) || (rc = unitig_cut_cycles(c, what, B, nn, &cur, &rounds, open))) return rc;
    tr.mark(c->stream);
    // layout: start nodes and their node counts (link is free now), their scans (joined is free now)
    const u32 *ptr = B.ptr[cur], *dist = B.dist[cur];
    u32 *is_first = link, *first_len = link + nn, *cid_of = joined, *poff_of = joined + nn;
    hipLaunchKernelGGL(kmc_contig_place_kernel, blocks(nn), dim3(KMC_CT_THREADS), 0, c->stream, nn, ptr, dist, is_first, first_len);
    launch_exclusive_scan<0>(c->stream, is_first, (u32)nn, (u32*)c->c_bsum.p, cid_of, (u32*)(ctl + KMC_CT_SCAN_C));
    launch_exclusive_scan<0>(c->stream, first_len, (u32)nn, (u32*)c->c_bsum.p, poff_of, (u32*)(ctl + KMC_CT_SCAN_P));
    if ((rc = read_ctl())) return rc;
    const u64 nc = w[KMC_CT_SCAN_C] & 0xFFFFFFFFull;
    if ((w[KMC_CT_SCAN_P] & 0xFFFFFFFFull) != nn || !nc || nc > nn)
        return fail(c, KMC_ERR_HIP, "internal error: %s laid out %llu of %llu nodes in %llu contigs", what, (unsigned long long)(w[KMC_CT_SCAN_P] & 0xFFFFFFFFull),
                    (unsigned long long)nn, (unsigned long long)nc);
    if ((rc = ensure(c, c->ct_poffs, (size_t)(nc + 1) * sizeof(u64))) || (rc = ensure(c, c->ct_offs, (size_t)(nc + 1) * sizeof(u64))) ||
        (rc = ensure(c, c->ct_abund, (size_t)nc * sizeof(u64))) || (rc = ensure(c, c->ct_flags, (size_t)std::max<u64>(nc, 8))) ||
        (rc = ensure(c, c->ct_path, (size_t)nn * sizeof(u32))) || (rc = ensure(c, c->ct_cid, (size_t)nn * sizeof(u32))) ||
        (rc = ensure(c, c->ct_keys, (size_t)nn * sizeof(u32))) || (rc = ensure(c, c->ct_g, (size_t)nn * sizeof(u32))) ||
        (rc = ensure(c, c->ct_start, (size_t)(nn + 1) * sizeof(u64))) || (rc = ensure(c, c->ct_src, (size_t)nn * sizeof(u64))))
        return rc;
    HIPCHK(c, hipMemsetAsync(c->ct_abund.p, 0, (size_t)nc * sizeof(u64), c->stream));
    ContigSrc S;
    S.u_offs = (const u64*)c->u_offs.p; S.u_abund = (const kmc_ull*)c->u_abund.p; S.n_unitigs = nu; S.u_bases = u_nb;
    hipLaunchKernelGGL(kmc_contig_path_kernel, blocks(nn), dim3(KMC_CT_THREADS), 0, c->stream, nn, nc, k, ptr, dist, (const u32*)cid_of, (const u32*)poff_of,
                       (const uint8_t*)c->ct_circ.p, owner, S, (u32*)c->ct_path.p, (u32*)c->ct_cid.p, (u32*)c->ct_keys.p, (u64*)c->ct_src.p,
                       (u64*)c->ct_poffs.p, (kmc_ull*)c->ct_abund.p, (uint8_t*)c->ct_flags.p, ctl);
    launch_exclusive_scan<0>(c->stream, c->ct_keys.p, (u32)nn, (u32*)c->c_bsum.p, (u32*)c->ct_g.p, (u32*)(ctl + KMC_CT_SCAN_G));
    if ((rc = read_ctl())) return rc;
    const u64 nk = w[KMC_CT_KEYS], nb = nk + nc * (u64)(k - 1);
    if (nk >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: 2^32 keys or more over the paths", what);
    if ((w[KMC_CT_SCAN_G] & 0xFFFFFFFFull) != nk)
        return fail(c, KMC_ERR_HIP, "internal error: %s scanned %llu of %llu keys", what, (unsigned long long)(w[KMC_CT_SCAN_G] & 0xFFFFFFFFull), (unsigned long long)nk);
    if ((rc = ensure(c, c->ct_bases, (size_t)nb + 64))) return rc;
    hipLaunchKernelGGL(kmc_contig_starts_kernel, blocks(nn), dim3(KMC_CT_THREADS), 0, c->stream, nn, nc, k, nb, (const u32*)c->ct_g.p, (const u32*)c->ct_cid.p,
                       (const u64*)c->ct_poffs.p, (u64*)c->ct_start.p, (u64*)c->ct_offs.p, ctl);
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    // emit (d_bases is readable up to the next 16-byte boundary: the rule of kmc_add_batch_device)
    hipLaunchKernelGGL(kmc_contig_emit_kernel, blocks((nb + 15) / 16), dim3(KMC_CT_THREADS), 0, c->stream, (const uint8_t*)c->u_bases.p, u_nb, nn, nb,
                       (const u64*)c->ct_start.p, (const u64*)c->ct_src.p, (const u32*)c->ct_path.p, (uint8_t*)c->ct_bases.p, ctl);
    tr.mark(c->stream);   // (as the trim call marks its gather: the kernel, not the copy of the control words and the wait)
    if ((rc = read_ctl())) return rc;
    h[0] = nc; h[1] = nn; h[2] = w[KMC_CT_DUP]; h[3] = w[KMC_CT_IGNORED]; h[4] = w[KMC_CT_CIRC]; h[5] = w[KMC_CT_ONE]; h[6] = w[KMC_CT_MOST]; h[7] = nb;
    if (tr.on && tr.n_ev == 5) {
        float ms[4] = {0, 0, 0, 0};
        bool ok = hipEventSynchronize(tr.ev[4]) == hipSuccess;
        for (int i = 0; ok && i < 4; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_unitig_contigs: unitigs %llu nodes %llu contigs %llu bases %llu rounds %u choice_ms %.4f rank_ms %.4f layout_ms %.4f emit_ms %.4f\n",
                    (unsigned long long)nu, (unsigned long long)nn, (unsigned long long)nc, (unsigned long long)nb, rounds, ms[0], ms[1], ms[2], ms[3]);
    }
    return KMC_OK;
}

// what both calls do once the state is in order: the held result (host form only) or a run that is kept
static int contigs_result(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, u64 min_reads, u64 min_support, bool may_reuse, u64* h) {
    min_reads = std::max<u64>(min_reads, 1);
    if (may_reuse && contigs_kept(c, min_count, max_count, min_reads, min_support)) {
        memcpy(h, c->ct_words, sizeof(c->ct_words));
        return KMC_OK;
    }
    if (int rc = contigs_run(c, what, min_reads, min_support, h)) return rc;
    c->ct_key.keep(c->view_gen, min_count, max_count);
    c->ct_reads = min_reads; c->ct_support = min_support;
    memcpy(c->ct_words, h, sizeof(c->ct_words));
    return KMC_OK;
}

static int kmc_unitig_contigs_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint64_t min_support,
                                          const void** d_bases, const void** d_offsets, const void** d_path_offsets, const void** d_path,
                                          const void** d_abund, const void** d_flags, uint64_t* n_contigs, uint64_t* n_nodes, uint64_t* n_bases,
                                          uint64_t* summary) {
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_unitig_contigs_device";
    u64 h[KMC_CONTIG_WORDS];
    int rc;
    if ((rc = contigs_begin(c, what, min_count, max_count)) || (rc = contigs_result(c, what, min_count, max_count, min_reads, min_support, false, h))) return rc;
    if (d_bases) *d_bases = c->ct_bases.p;
    if (d_offsets) *d_offsets = c->ct_offs.p;
    if (d_path_offsets) *d_path_offsets = c->ct_poffs.p;
    if (d_path) *d_path = c->ct_path.p;
    if (d_abund) *d_abund = c->ct_abund.p;
    if (d_flags) *d_flags = c->ct_flags.p;
    if (n_contigs) *n_contigs = h[0];
    if (n_nodes) *n_nodes = h[1];
    if (n_bases) *n_bases = h[7];
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

static int kmc_unitig_contigs_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint64_t min_support, uint8_t* bases,
                                   uint64_t cap_bases, uint64_t* offsets, uint64_t* path_offsets, uint64_t* abund, uint8_t* flags, uint64_t cap_contigs,
                                   uint32_t* path, uint64_t cap_nodes, uint64_t* n_contigs, uint64_t* n_nodes, uint64_t* n_bases, uint64_t* summary) {
    if (n_contigs) *n_contigs = 0;
    if (n_nodes) *n_nodes = 0;
    if (n_bases) *n_bases = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_unitig_contigs";
    u64 h[KMC_CONTIG_WORDS];
    int rc;
    if ((rc = contigs_begin(c, what, min_count, max_count)) || (rc = contigs_result(c, what, min_count, max_count, min_reads, min_support, true, h))) return rc;
    const u64 nc = h[0], nn = h[1], nb = h[7];
    if (n_contigs) *n_contigs = nc;
    if (n_nodes) *n_nodes = nn;
    if (n_bases) *n_bases = nb;
    if (bases && cap_bases < nb) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu bases", what, (unsigned long long)cap_bases, (unsigned long long)nb);
    if ((offsets || path_offsets || abund || flags) && cap_contigs < nc)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu contigs", what, (unsigned long long)cap_contigs, (unsigned long long)nc);
    if (path && cap_nodes < nn) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu nodes", what, (unsigned long long)cap_nodes, (unsigned long long)nn);
    if (bases && nb) HIPCHK(c, hipMemcpyAsync(bases, c->ct_bases.p, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    if (offsets) HIPCHK(c, hipMemcpyAsync(offsets, c->ct_offs.p, (size_t)(nc + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (path_offsets) HIPCHK(c, hipMemcpyAsync(path_offsets, c->ct_poffs.p, (size_t)(nc + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (abund && nc) HIPCHK(c, hipMemcpyAsync(abund, c->ct_abund.p, (size_t)nc * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (flags && nc) HIPCHK(c, hipMemcpyAsync(flags, c->ct_flags.p, (size_t)nc, hipMemcpyDeviceToHost, c->stream));
    if (path && nn) HIPCHK(c, hipMemcpyAsync(path, c->ct_path.p, (size_t)nn * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- reads corrected against the solid keys of the view: weak runs, candidates, replacements (kmc_correct.hip.h) ----
template <int PASS>
static void correct_runs_launch(kmc_ctx* c, const CorrBatch& b, u64 n_cands) {
    const u32 grid = (u32)std::min<u64>(b.n_tiles, (u64)c->n_cu * 8);
    hipLaunchKernelGGL(kmc_correct_runs_kernel<PASS>, dim3(grid), dim3(KMC_CR_THREADS), 0, c->stream, b, (u32*)c->c_tile.p, (const u32*)c->c_tpos.p,
                       n_cands, (uint4*)c->cr_cands.p, (u64*)c->cr_where.p, (u64*)c->cr_coffs.p, (u32*)c->cr_stats.p, (kmc_ull*)c->c_ctl.p);
}

// The batch (device arrays) corrected against the keys of this view inside the range, into the cr_* buffers;
// h[KMC_CORRECT_WORDS] the summary.  Finished when it returns.
static int correct_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, const uint8_t* d_bases, const u64* d_offsets, u64 n_reads,
                       u64 n_bases, u64* h, u64* n_cands) {
    memset(h, 0, KMC_CORRECT_WORDS * sizeof(u64));
    *n_cands = 0;
    int rc;
    const u64 n = c->n_sorted;
    const int k = c->klen;
    const u64 n_tiles = (n_bases + 1 + KMC_CR_TILE - 1) / KMC_CR_TILE;
    if (n_tiles >= (1ull << 31)) return fail(c, KMC_ERR_ARG, "%s: batch too large for one call", what);
    ChunkGrid g;
    if ((rc = chunk_grid(c, what, n_bases, k, &g))) return rc;
    const size_t stb = (size_t)std::max<u64>(n_reads, 1) * KMC_CORRECT_READ_WORDS * sizeof(u32);
    const size_t bitb = (size_t)std::max<u64>(g.n_chunks, 1) * 64 * sizeof(uint16_t);
    if ((rc = ensure(c, c->cr_out, (size_t)n_bases + 64)) || (rc = ensure(c, c->cr_stats, stb)) ||
        (rc = ensure(c, c->cr_coffs, (size_t)(n_reads + 1) * sizeof(u64))) || (rc = ensure(c, c->cr_cands, 16)) || (rc = ensure(c, c->cr_where, 16)) ||
        (rc = ensure(c, c->cr_sbits, bitb)) || (rc = ensure(c, c->cr_vbits, bitb)) || (rc = ensure(c, c->cr_wbits, bitb)) ||
        (rc = compact_plan(c, n_tiles, KMC_CR_CTL_WORDS)))
        return rc;
    HIPCHK(c, hipMemsetAsync(c->cr_stats.p, 0, stb, c->stream));
    if (!n_reads) {
        HIPCHK(c, hipMemsetAsync(c->cr_coffs.p, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KMC_OK;
    }
    QView v;
    if ((rc = query_view(c, what, &v))) return rc;
    kmc_ull* ctl = (kmc_ull*)c->c_ctl.p;
    const u64 lo_c = std::max<u64>(min_count, 1), hi_c = count_hi(max_count);
    // the copy that takes the corrections (a caller may hand the last call's own result back in)
    if (n_bases && (const void*)d_bases != c->cr_out.p) HIPCHK(c, hipMemcpyAsync(c->cr_out.p, d_bases, (size_t)n_bases, hipMemcpyDeviceToDevice, c->stream));
    UnitigTrace tr;
    tr.mark(c->stream);
    if (g.n_chunks) with_kw_canon(c, [&](auto KW, auto CANON) {
        hipLaunchKernelGGL((kmc_correct_mark_kernel<KW(), CANON()>), dim3((u32)g.grid), dim3(KMC_Q_THREADS), 0, c->stream, d_bases, n_bases, d_offsets,
                           n_reads, k, g.n_chunks, g.cpw, v, lo_c, hi_c, (uint16_t*)c->cr_sbits.p, (uint16_t*)c->cr_vbits.p, (uint16_t*)c->cr_wbits.p);
    });
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    CorrBatch b;
    b.start_bits = (const uint16_t*)c->cr_sbits.p; b.valid_bits = (const uint16_t*)c->cr_vbits.p; b.weak_bits = (const uint16_t*)c->cr_wbits.p;
    b.bases = d_bases; b.offsets = d_offsets; b.n_reads = n_reads; b.n_bases = n_bases; b.n_words = g.n_chunks * 64; b.n_tiles = n_tiles; b.k = k;
    correct_runs_launch<0>(c, b, 0);
    u64 w[KMC_CR_CTL_WORDS];
    if ((rc = compact_scan_and_read(c, n_tiles, w, KMC_CR_CTL_WORDS))) return rc;
    const u64 nc = w[KMC_CR_CANDS];
    if (nc >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: 2^32 candidates or more", what);
    if ((w[0] & 0xFFFFFFFFull) != nc)
        return fail(c, KMC_ERR_HIP, "internal error: %s scanned %llu of %llu candidates", what, (unsigned long long)(w[0] & 0xFFFFFFFFull), (unsigned long long)nc);
    if ((rc = ensure(c, c->cr_cands, (size_t)std::max<u64>(nc, 1) * 4 * sizeof(u32))) || (rc = ensure(c, c->cr_where, (size_t)std::max<u64>(nc, 1) * 2 * sizeof(u64))))
        return rc;
    correct_runs_launch<1>(c, b, nc);
    hipLaunchKernelGGL(kmc_correct_reads_kernel, dim3((u32)grid_for(c, n_reads, KMC_CR_THREADS)), dim3(KMC_CR_THREADS), 0, c->stream, d_offsets, n_reads, ctl);
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    if (nc) with_kw_canon(c, [&](auto KW, auto CANON) {
        const u32 grid = (u32)std::min<u64>((nc + KMC_CR_WAVES - 1) / KMC_CR_WAVES, (u64)c->n_cu * 16);
        hipLaunchKernelGGL((kmc_correct_try_kernel<KW(), CANON()>), dim3(grid), dim3(KMC_CR_THREADS), 0, c->stream, d_bases, n_bases, n_reads, k, v, lo_c,
                           hi_c, nc, (uint4*)c->cr_cands.p, (const u64*)c->cr_where.p, (uint8_t*)c->cr_out.p, (u32*)c->cr_stats.p, ctl);
    });
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[KMC_CR_BAD]) return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays", what, (unsigned long long)w[KMC_CR_BAD]);
    if (w[KMC_CR_LONG]) return fail(c, KMC_ERR_ARG, "%s: %llu reads of 2^32 bases or more", what, (unsigned long long)w[KMC_CR_LONG]);
    h[0] = n_reads; h[1] = w[KMC_CR_VALID]; h[2] = w[KMC_CR_WEAK]; h[3] = w[KMC_CR_RUNS]; h[4] = nc; h[5] = w[KMC_CR_FIXED]; h[6] = w[KMC_CR_AMBIG];
    h[7] = w[KMC_CR_WEAK] - w[KMC_CR_FIXED_WIN];
    *n_cands = nc;
    if (tr.on && tr.n_ev == 4) {
        float ms[3] = {0, 0, 0};
        bool ok = hipEventSynchronize(tr.ev[3]) == hipSuccess;
        for (int i = 0; ok && i < 3; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_correct: keys %llu reads %llu windows %llu weak %llu runs %llu cands %llu fixed %llu mark_ms %.4f runs_ms %.4f try_ms %.4f\n",
                    (unsigned long long)n, (unsigned long long)n_reads, (unsigned long long)h[1], (unsigned long long)h[2], (unsigned long long)h[3],
                    (unsigned long long)nc, (unsigned long long)h[5], ms[0], ms[1], ms[2]);
    }
    return KMC_OK;
}

static int kmc_correct_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void* d_bases, const void* d_offsets, uint64_t n_reads,
                                   uint64_t n_bases, const void** d_corrected, const void** d_read_stats, const void** d_cand_offsets,
                                   const void** d_cands, uint64_t* n_cands, uint64_t* summary) {
    if (n_cands) *n_cands = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_correct_device";
    int rc;
    if ((rc = graph_begin(c, what, min_count, max_count))) return rc;
    if (n_reads && (rc = check_device_batch(c, what, d_bases, d_offsets))) return rc;
    u64 h[KMC_CORRECT_WORDS], nc = 0;
    if ((rc = correct_run(c, what, min_count, max_count, (const uint8_t*)d_bases, (const u64*)d_offsets, n_reads, n_reads ? n_bases : 0, h, &nc))) return rc;
    if (d_corrected) *d_corrected = c->cr_out.p;
    if (d_read_stats) *d_read_stats = c->cr_stats.p;
    if (d_cand_offsets) *d_cand_offsets = c->cr_coffs.p;
    if (d_cands) *d_cands = c->cr_cands.p;
    if (n_cands) *n_cands = nc;
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

static int kmc_correct_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                            uint8_t* out_bases, uint32_t* read_stats, uint64_t* cand_offsets, uint32_t* cands, uint64_t cap_cands,
                            uint64_t* n_cands, uint64_t* summary) {
    if (n_cands) *n_cands = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_correct";
    int rc;
    if ((rc = graph_begin(c, what, min_count, max_count))) return rc;
    u64 n_bases = 0;
    if (n_reads && (rc = stage_batch(c, what, bases, offsets, n_reads, true, &n_bases))) return rc;
    u64 h[KMC_CORRECT_WORDS], nc = 0;
    if ((rc = correct_run(c, what, min_count, max_count, (const uint8_t*)c->q_bases.p, (const u64*)c->q_offs.p, n_reads, n_bases, h, &nc))) return rc;
    if (n_cands) *n_cands = nc;
    if (cands && cap_cands < nc) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu candidates", what, (unsigned long long)cap_cands, (unsigned long long)nc);
    if (out_bases && n_bases) HIPCHK(c, hipMemcpyAsync(out_bases, c->cr_out.p, (size_t)n_bases, hipMemcpyDeviceToHost, c->stream));
    if (read_stats && n_reads) HIPCHK(c, hipMemcpyAsync(read_stats, c->cr_stats.p, (size_t)n_reads * KMC_CORRECT_READ_WORDS * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    if (cand_offsets) HIPCHK(c, hipMemcpyAsync(cand_offsets, c->cr_coffs.p, (size_t)(n_reads + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (cands && nc) HIPCHK(c, hipMemcpyAsync(cands, c->cr_cands.p, (size_t)nc * 4 * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- reads trimmed and filtered by their strong windows: runs per read, verdicts, the emitted spans as a batch (kmc_trim.hip.h) ----
// the rule arguments of both calls (kmc.h: SPAN, PASS, PAIRS, INVERT)
static int trim_rule(kmc_ctx* c, const char* what, int mode, uint32_t flags, uint64_t min_strong, uint32_t min_permille, uint64_t min_len,
                     uint64_t n_reads, TrimRule* R) {
    if (mode != KMC_TRIM_NONE && mode != KMC_TRIM_ENDS && mode != KMC_TRIM_LONGEST) return fail(c, KMC_ERR_ARG, "%s: unknown mode %d", what, mode);
    if (flags & ~(KMC_TRIM_INVERT | KMC_TRIM_PAIR_BOTH | KMC_TRIM_PAIR_EITHER)) return fail(c, KMC_ERR_ARG, "%s: unknown flag bits 0x%x", what, flags);
    if ((flags & KMC_TRIM_PAIR_BOTH) && (flags & KMC_TRIM_PAIR_EITHER)) return fail(c, KMC_ERR_ARG, "%s: KMC_TRIM_PAIR_BOTH and KMC_TRIM_PAIR_EITHER exclude each other", what);
    if ((flags & (KMC_TRIM_PAIR_BOTH | KMC_TRIM_PAIR_EITHER)) && (n_reads & 1))
        return fail(c, KMC_ERR_ARG, "%s: %llu reads cannot be pairs", what, (unsigned long long)n_reads);
    if ((flags & KMC_TRIM_INVERT) && mode != KMC_TRIM_NONE) return fail(c, KMC_ERR_ARG, "%s: KMC_TRIM_INVERT needs KMC_TRIM_NONE", what);
    if (min_permille > 1000) return fail(c, KMC_ERR_ARG, "%s: min_permille %u > 1000", what, min_permille);
    R->mode = mode; R->k = c->klen; R->flags = flags; R->min_permille = min_permille; R->min_strong = min_strong; R->min_len = min_len;
    return KMC_OK;
}

// The batch (device arrays) judged against the keys of this view inside the range, into the tr_* buffers; h[KMC_TRIM_WORDS]
// the summary.  Finished when it returns.
static int trim_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, const TrimRule& R, const uint8_t* d_bases, const u64* d_offsets,
                    u64 n_reads, u64 n_bases, u64* h) {
    memset(h, 0, KMC_TRIM_WORDS * sizeof(u64));
    int rc;
    const u64 n = c->n_sorted;
    const int k = c->klen;
    // the scans of kmc_scan.hip.h work on u32: positions among the reads and among the emitted bases
    if (n_reads >= (1ull << 31) || n_bases >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: a batch of 2^31 reads or 2^32 bases or more", what);
    ChunkGrid g;
    if ((rc = chunk_grid(c, what, n_bases, k, &g))) return rc;
    const int cur = c->tr_cur ^ 1;   // the last call's result stays readable while this one is written
    const u64 nr1 = std::max<u64>(n_reads, 1);
    const size_t bitb = (size_t)std::max<u64>(g.n_chunks, 1) * 64 * sizeof(uint16_t), w32 = (size_t)nr1 * sizeof(u32);
    const size_t scan_blocks = (size_t)((n_reads + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK);
    if ((rc = ensure(c, c->tr_out[cur], (size_t)n_bases + 64)) || (rc = ensure(c, c->tr_ooffs[cur], (size_t)(n_reads + 1) * sizeof(u64))) ||
        (rc = ensure(c, c->tr_origin, (size_t)nr1 * sizeof(u64))) || (rc = ensure(c, c->tr_stats, (size_t)nr1 * KMC_TRIM_READ_WORDS * sizeof(u32))) ||
        (rc = ensure(c, c->tr_verdict, (size_t)nr1)) || (rc = ensure(c, c->tr_sbits, bitb)) || (rc = ensure(c, c->tr_vbits, bitb)) ||
        (rc = ensure(c, c->tr_wbits, bitb)) || (rc = ensure(c, c->tr_runs, (size_t)nr1 * 2 * sizeof(uint4))) || (rc = ensure(c, c->tr_list, w32)) ||
        (rc = ensure(c, c->tr_emit, w32)) || (rc = ensure(c, c->tr_elen, w32)) || (rc = ensure(c, c->tr_epos, w32)) || (rc = ensure(c, c->tr_lpos, w32)) ||
        (rc = ensure(c, c->tr_src, (size_t)nr1 * sizeof(u64))) || (rc = ensure(c, c->c_bsum, (scan_blocks + 2) * sizeof(u32))) ||
        (rc = ensure(c, c->c_ctl, KMC_TR_CTL_WORDS * sizeof(u64))))
        return rc;
    c->tr_cur = cur;
    if (!n_reads) {
        HIPCHK(c, hipMemsetAsync(c->tr_ooffs[cur].p, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KMC_OK;
    }
    QView v;
    if ((rc = query_view(c, what, &v))) return rc;
    kmc_ull* ctl = (kmc_ull*)c->c_ctl.p;
    HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_TR_CTL_WORDS * sizeof(u64), c->stream));
    const u64 lo_c = std::max<u64>(min_count, 1), hi_c = count_hi(max_count);
    UnitigTrace tr;
    tr.mark(c->stream);
    if (g.n_chunks) with_kw_canon(c, [&](auto KW, auto CANON) {
        hipLaunchKernelGGL((kmc_correct_mark_kernel<KW(), CANON()>), dim3((u32)g.grid), dim3(KMC_Q_THREADS), 0, c->stream, d_bases, n_bases, d_offsets,
                           n_reads, k, g.n_chunks, g.cpw, v, lo_c, hi_c, (uint16_t*)c->tr_sbits.p, (uint16_t*)c->tr_vbits.p, (uint16_t*)c->tr_wbits.p);
    });
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    TrimBits B;
    B.valid = (const u64*)c->tr_vbits.p; B.weak = (const u64*)c->tr_wbits.p; B.n_words = g.n_chunks * 16;
    const u32 rgrid = (u32)grid_for(c, n_reads, KMC_TR_THREADS), ggrid = (u32)std::min<u64>(n_reads, (u64)c->n_cu * 8);
    uint4* runs = (uint4*)c->tr_runs.p;
    hipLaunchKernelGGL(kmc_trim_reduce_kernel, dim3(rgrid), dim3(KMC_TR_THREADS), 0, c->stream, B, d_offsets, n_reads, n_bases, k, runs, (u32*)c->tr_list.p, ctl);
    hipLaunchKernelGGL(kmc_trim_reduce_group_kernel<64>, dim3(ggrid), dim3(KMC_TR_THREADS), 0, c->stream, B, d_offsets, n_reads, n_bases, k, runs,
                       (const u32*)c->tr_list.p, ctl);
    hipLaunchKernelGGL(kmc_trim_reduce_group_kernel<KMC_TR_THREADS>, dim3(ggrid), dim3(KMC_TR_THREADS), 0, c->stream, B, d_offsets, n_reads, n_bases, k,
                       runs, (const u32*)c->tr_list.p, ctl);
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    hipLaunchKernelGGL(kmc_trim_verdict_kernel, dim3(rgrid), dim3(KMC_TR_THREADS), 0, c->stream, R, (const uint4*)runs, d_offsets, n_reads, n_bases,
                       (uint4*)c->tr_stats.p, (uint8_t*)c->tr_verdict.p, (u32*)c->tr_emit.p, (u32*)c->tr_elen.p, ctl);
    launch_exclusive_scan<0>(c->stream, c->tr_emit.p, (u32)n_reads, (u32*)c->c_bsum.p, (u32*)c->tr_epos.p, (u32*)(ctl + KMC_TR_N_OUT));
    launch_exclusive_scan<0>(c->stream, c->tr_elen.p, (u32)n_reads, (u32*)c->c_bsum.p, (u32*)c->tr_lpos.p, (u32*)(ctl + KMC_TR_N_BASES));
    hipLaunchKernelGGL(kmc_trim_layout_kernel<false>, dim3(rgrid), dim3(KMC_TR_THREADS), 0, c->stream, (const uint4*)c->tr_stats.p, d_offsets, n_reads,
                       (const u32*)c->tr_emit.p, (const u32*)c->tr_elen.p, (const u32*)c->tr_epos.p, (const u32*)c->tr_lpos.p, (u64*)c->tr_ooffs[cur].p,
                       (u64*)c->tr_origin.p, (u64*)c->tr_src.p, ctl);
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    if (n_bases) {
        // the emitted bases are at most the batch's: a lane per 16 of those, the ones past the scan's total leave at once
        const u64 blocks = ((n_bases + 15) / 16 + KMC_TR_THREADS - 1) / KMC_TR_THREADS;
        hipLaunchKernelGGL(kmc_trim_gather_kernel, dim3((u32)blocks), dim3(KMC_TR_THREADS), 0, c->stream, d_bases, n_bases, n_reads,
                           (const u64*)c->tr_ooffs[cur].p, (const u64*)c->tr_src.p, (uint8_t*)c->tr_out[cur].p, ctl);
        HIPCHK(c, hipGetLastError());
    }
    tr.mark(c->stream);
    u64 w[KMC_TR_CTL_WORDS];
    HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[KMC_TR_LONG]) return fail(c, KMC_ERR_ARG, "%s: %llu reads of 2^32 bases or more", what, (unsigned long long)w[KMC_TR_LONG]);
    if (w[KMC_TR_BAD]) return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays", what, (unsigned long long)w[KMC_TR_BAD]);
    if (w[KMC_TR_N_OUT] != w[KMC_TR_EMITTED] || w[KMC_TR_N_BASES] != w[KMC_TR_BASES])
        return fail(c, KMC_ERR_HIP, "internal error: %s scanned %llu reads and %llu bases of %llu and %llu", what, (unsigned long long)w[KMC_TR_N_OUT],
                    (unsigned long long)w[KMC_TR_N_BASES], (unsigned long long)w[KMC_TR_EMITTED], (unsigned long long)w[KMC_TR_BASES]);
    h[0] = n_reads; h[1] = w[KMC_TR_VALID]; h[2] = w[KMC_TR_STRONG]; h[3] = w[KMC_TR_PASSED]; h[4] = w[KMC_TR_EMITTED]; h[5] = w[KMC_TR_BASES];
    h[6] = w[KMC_TR_CUT]; h[7] = w[KMC_TR_BEFORE];
    if (tr.on && tr.n_ev == 5) {
        float ms[4] = {0, 0, 0, 0};
        bool ok = hipEventSynchronize(tr.ev[4]) == hipSuccess;
        for (int i = 0; ok && i < 4; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_trim: keys %llu reads %llu windows %llu strong %llu passed %llu emitted %llu bases %llu mark_ms %.4f reduce_ms %.4f "
                    "layout_ms %.4f gather_ms %.4f\n", (unsigned long long)n, (unsigned long long)n_reads, (unsigned long long)h[1], (unsigned long long)h[2],
                    (unsigned long long)h[3], (unsigned long long)h[4], (unsigned long long)h[5], ms[0], ms[1], ms[2], ms[3]);
    }
    return KMC_OK;
}

static int kmc_trim_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, int mode, uint32_t flags, uint64_t min_strong,
                                uint32_t min_permille, uint64_t min_len, const void* d_bases, const void* d_offsets, uint64_t n_reads,
                                uint64_t n_bases, const void** d_out_bases, const void** d_out_offsets, const void** d_origin,
                                const void** d_read_stats, const void** d_verdict, uint64_t* n_out, uint64_t* n_out_bases, uint64_t* summary) {
    if (n_out) *n_out = 0;
    if (n_out_bases) *n_out_bases = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_trim_device";
    int rc;
    TrimRule R;
    if ((rc = graph_begin(c, what, min_count, max_count)) || (rc = trim_rule(c, what, mode, flags, min_strong, min_permille, min_len, n_reads, &R))) return rc;
    if (n_reads && (rc = check_device_batch(c, what, d_bases, d_offsets))) return rc;
    u64 h[KMC_TRIM_WORDS];
    if ((rc = trim_run(c, what, min_count, max_count, R, (const uint8_t*)d_bases, (const u64*)d_offsets, n_reads, n_reads ? n_bases : 0, h))) return rc;
    if (d_out_bases) *d_out_bases = c->tr_out[c->tr_cur].p;
    if (d_out_offsets) *d_out_offsets = c->tr_ooffs[c->tr_cur].p;
    if (d_origin) *d_origin = c->tr_origin.p;
    if (d_read_stats) *d_read_stats = c->tr_stats.p;
    if (d_verdict) *d_verdict = c->tr_verdict.p;
    if (n_out) *n_out = h[4];
    if (n_out_bases) *n_out_bases = h[5];
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

static int kmc_trim_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, int mode, uint32_t flags, uint64_t min_strong, uint32_t min_permille,
                         uint64_t min_len, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint8_t* out_bases, uint64_t cap_bases,
                         uint64_t* out_offsets, uint64_t* origin, uint64_t cap_reads, uint32_t* read_stats, uint8_t* verdict, uint64_t* n_out,
                         uint64_t* n_out_bases, uint64_t* summary) {
    if (n_out) *n_out = 0;
    if (n_out_bases) *n_out_bases = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_trim";
    int rc;
    TrimRule R;
    if ((rc = graph_begin(c, what, min_count, max_count)) || (rc = trim_rule(c, what, mode, flags, min_strong, min_permille, min_len, n_reads, &R))) return rc;
    u64 n_bases = 0;
    if (n_reads && (rc = stage_batch(c, what, bases, offsets, n_reads, true, &n_bases))) return rc;
    u64 h[KMC_TRIM_WORDS];
    if ((rc = trim_run(c, what, min_count, max_count, R, (const uint8_t*)c->q_bases.p, (const u64*)c->q_offs.p, n_reads, n_bases, h))) return rc;
    const u64 no = h[4], nb = h[5];
    if (n_out) *n_out = no;
    if (n_out_bases) *n_out_bases = nb;
    if (out_bases && cap_bases < nb) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu bases", what, (unsigned long long)cap_bases, (unsigned long long)nb);
    if ((out_offsets || origin) && cap_reads < no) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu reads", what, (unsigned long long)cap_reads, (unsigned long long)no);
    const int cur = c->tr_cur;
    if (out_bases && nb) HIPCHK(c, hipMemcpyAsync(out_bases, c->tr_out[cur].p, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    if (out_offsets) HIPCHK(c, hipMemcpyAsync(out_offsets, c->tr_ooffs[cur].p, (size_t)(no + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (origin && no) HIPCHK(c, hipMemcpyAsync(origin, c->tr_origin.p, (size_t)no * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (read_stats && n_reads) HIPCHK(c, hipMemcpyAsync(read_stats, c->tr_stats.p, (size_t)n_reads * KMC_TRIM_READ_WORDS * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    if (verdict && n_reads) HIPCHK(c, hipMemcpyAsync(verdict, c->tr_verdict.p, (size_t)n_reads, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- read depth normalised: a depth per read, verdicts, the emitted reads as a batch (kmc_normalize.hip.h) ----
// the rule arguments of both calls (kmc.h: DEPTH, UNIT, LOW, DEEP, KEEP)
static int normalize_rule(kmc_ctx* c, const char* what, uint32_t permille, uint64_t target, uint64_t min_depth, uint64_t seed, uint32_t flags,
                          uint64_t n_reads, NormRule* R) {
    if (permille > 1000) return fail(c, KMC_ERR_ARG, "%s: permille %u > 1000", what, permille);
    if (flags & ~(KMC_NORM_PAIRED | KMC_NORM_INVERT)) return fail(c, KMC_ERR_ARG, "%s: unknown flag bits 0x%x", what, flags);
    if ((flags & KMC_NORM_PAIRED) && (n_reads & 1)) return fail(c, KMC_ERR_ARG, "%s: %llu reads cannot be pairs", what, (unsigned long long)n_reads);
    R->permille = permille; R->flags = flags; R->target = target; R->min_depth = min_depth; R->seed = seed;
    return KMC_OK;
}

// does the array that begins at p lie in b?
static bool inside(const DevBuf& b, const void* p) {
    return b.p && p && (uintptr_t)p >= (uintptr_t)b.p && (uintptr_t)p < (uintptr_t)b.p + b.bytes;
}

// The batch (device arrays) judged against this view, into the nm_* buffers; h[KMC_NORMALIZE_WORDS] the summary.  Finished
// when it returns.
static int normalize_run(kmc_ctx* c, const char* what, const NormRule& R, const uint8_t* d_bases, const u64* d_offsets, u64 n_reads, u64 n_bases,
                         u64* h) {
    memset(h, 0, KMC_NORMALIZE_WORDS * sizeof(u64));
    int rc;
    const u64 n = c->n_sorted;
    const int k = c->klen;
    // the scans of kmc_scan.hip.h work on u32: positions among the reads and among the emitted bases
    if (n_reads >= (1ull << 31) || n_bases >= (1ull << 32)) return fail(c, KMC_ERR_CAPACITY, "%s: a batch of 2^31 reads or 2^32 bases or more", what);
    // the call writes these while it still reads the batch
    if (n_reads && (inside(c->nm_out, d_bases) || inside(c->nm_ooffs, d_offsets)))
        return fail(c, KMC_ERR_ARG, "%s: the input is this ctx's own kmc_normalize result", what);
    const u64 nr1 = std::max<u64>(n_reads, 1);
    const size_t w32 = (size_t)nr1 * sizeof(u32);
    const size_t scan_blocks = (size_t)((n_reads + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK);
    if ((rc = ensure(c, c->nm_out, (size_t)n_bases + 64)) || (rc = ensure(c, c->nm_ooffs, (size_t)(n_reads + 1) * sizeof(u64))) ||
        (rc = ensure(c, c->nm_origin, (size_t)nr1 * sizeof(u64))) || (rc = ensure(c, c->nm_stats, (size_t)nr1 * KMC_NORMALIZE_READ_WORDS * sizeof(u32))) ||
        (rc = ensure(c, c->nm_verdict, (size_t)nr1)) || (rc = ensure(c, c->nm_win, (size_t)std::max<u64>(n_bases, 1) * sizeof(u32))) ||
        (rc = ensure(c, c->nm_pstats, (size_t)nr1 * KMC_PROFILE_WORDS * sizeof(u64))) || (rc = ensure(c, c->nm_depth, w32)) ||
        (rc = ensure(c, c->nm_list, w32)) || (rc = ensure(c, c->nm_emit, w32)) || (rc = ensure(c, c->nm_elen, w32)) || (rc = ensure(c, c->nm_epos, w32)) ||
        (rc = ensure(c, c->nm_lpos, w32)) || (rc = ensure(c, c->nm_src, (size_t)nr1 * sizeof(u64))) ||
        (rc = ensure(c, c->c_bsum, (scan_blocks + 2) * sizeof(u32))) || (rc = ensure(c, c->c_ctl, KMC_NM_CTL_WORDS * sizeof(u64))))
        return rc;
    if (!n_reads) {
        HIPCHK(c, hipMemsetAsync(c->nm_ooffs.p, 0, sizeof(u64), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KMC_OK;
    }
    kmc_ull* ctl = (kmc_ull*)c->c_ctl.p;
    HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_NM_CTL_WORDS * sizeof(u64), c->stream));
    UnitigTrace tr;
    tr.mark(c->stream);
    const u32* win = (const u32*)c->nm_win.p;
    const kmc_ull* pstats = (const kmc_ull*)c->nm_pstats.p;
    if ((rc = profile_launch(c, d_bases, d_offsets, n_reads, n_bases, 1, (u32*)c->nm_win.p, (u64*)c->nm_pstats.p))) return rc;
    tr.mark(c->stream);
    const u32 rgrid = (u32)grid_for(c, n_reads, KMC_NM_THREADS), ggrid = (u32)std::min<u64>(n_reads, (u64)c->n_cu * 8);
    // a wave takes KMC_NM_TRIP reads per trip and selects them one after the other: a workgroup per trip, up to 16 per CU
    const u64 per_wg = (u64)KMC_NM_WAVES * KMC_NM_TRIP;
    const u32 sgrid = (u32)std::min<u64>((n_reads + per_wg - 1) / per_wg, (u64)c->n_cu * 16);
    hipLaunchKernelGGL(kmc_normalize_select_kernel, dim3(sgrid), dim3(KMC_NM_THREADS), 0, c->stream, win, pstats, d_offsets, n_reads, n_bases, k,
                       R.permille, (u32*)c->nm_depth.p, (u32*)c->nm_list.p, ctl);
    hipLaunchKernelGGL(kmc_normalize_select_group_kernel, dim3(ggrid), dim3(KMC_NM_THREADS), 0, c->stream, win, pstats, d_offsets, n_reads, n_bases, k,
                       R.permille, (u32*)c->nm_depth.p, (const u32*)c->nm_list.p, ctl);
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    hipLaunchKernelGGL(kmc_normalize_verdict_kernel, dim3(rgrid), dim3(KMC_NM_THREADS), 0, c->stream, R, (const u32*)c->nm_depth.p, pstats, d_offsets,
                       n_reads, (uint4*)c->nm_stats.p, (uint8_t*)c->nm_verdict.p, (u32*)c->nm_emit.p, (u32*)c->nm_elen.p, ctl);
    launch_exclusive_scan<0>(c->stream, c->nm_emit.p, (u32)n_reads, (u32*)c->c_bsum.p, (u32*)c->nm_epos.p, (u32*)(ctl + KMC_NM_N_OUT));
    launch_exclusive_scan<0>(c->stream, c->nm_elen.p, (u32)n_reads, (u32*)c->c_bsum.p, (u32*)c->nm_lpos.p, (u32*)(ctl + KMC_NM_N_BASES));
    hipLaunchKernelGGL(kmc_trim_layout_kernel<true>, dim3(rgrid), dim3(KMC_NM_THREADS), 0, c->stream, (const uint4*)c->nm_stats.p, d_offsets, n_reads,
                       (const u32*)c->nm_emit.p, (const u32*)c->nm_elen.p, (const u32*)c->nm_epos.p, (const u32*)c->nm_lpos.p, (u64*)c->nm_ooffs.p,
                       (u64*)c->nm_origin.p, (u64*)c->nm_src.p, ctl);
    HIPCHK(c, hipGetLastError());
    tr.mark(c->stream);
    if (n_bases) {
        // the emitted bases are at most the batch's: a lane per 16 of those, the ones past the scan's total leave at once
        const u64 blocks = ((n_bases + 15) / 16 + KMC_NM_THREADS - 1) / KMC_NM_THREADS;
        hipLaunchKernelGGL(kmc_trim_gather_kernel, dim3((u32)blocks), dim3(KMC_NM_THREADS), 0, c->stream, d_bases, n_bases, n_reads,
                           (const u64*)c->nm_ooffs.p, (const u64*)c->nm_src.p, (uint8_t*)c->nm_out.p, ctl);
        HIPCHK(c, hipGetLastError());
    }
    tr.mark(c->stream);
    u64 w[KMC_NM_CTL_WORDS];
    HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[KMC_NM_LONG]) return fail(c, KMC_ERR_ARG, "%s: %llu reads of 2^32 bases or more", what, (unsigned long long)w[KMC_NM_LONG]);
    if (w[KMC_NM_BAD]) return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays", what, (unsigned long long)w[KMC_NM_BAD]);
    if (w[KMC_NM_N_OUT] != w[KMC_NM_EMITTED] || w[KMC_NM_N_BASES] != w[KMC_NM_BASES])
        return fail(c, KMC_ERR_HIP, "internal error: %s scanned %llu reads and %llu bases of %llu and %llu", what, (unsigned long long)w[KMC_NM_N_OUT],
                    (unsigned long long)w[KMC_NM_N_BASES], (unsigned long long)w[KMC_NM_EMITTED], (unsigned long long)w[KMC_NM_BASES]);
    h[0] = n_reads; h[1] = w[KMC_NM_VALID]; h[2] = w[KMC_NM_EMITTED]; h[3] = w[KMC_NM_BASES]; h[4] = w[KMC_NM_LOW]; h[5] = w[KMC_NM_DEEP];
    h[6] = w[KMC_NM_DEEP_KEPT]; h[7] = w[KMC_NM_DSUM];
    if (tr.on && tr.n_ev == 5) {
        float ms[4] = {0, 0, 0, 0};
        bool ok = hipEventSynchronize(tr.ev[4]) == hipSuccess;
        for (int i = 0; ok && i < 4; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_normalize: keys %llu reads %llu windows %llu emitted %llu bases %llu low %llu deep %llu kept %llu profile_ms %.4f "
                    "select_ms %.4f layout_ms %.4f gather_ms %.4f\n", (unsigned long long)n, (unsigned long long)n_reads, (unsigned long long)h[1],
                    (unsigned long long)h[2], (unsigned long long)h[3], (unsigned long long)h[4], (unsigned long long)h[5], (unsigned long long)h[6],
                    ms[0], ms[1], ms[2], ms[3]);
    }
    return KMC_OK;
}

static int kmc_normalize_device_impl(kmc_ctx* c, uint32_t permille, uint64_t target, uint64_t min_depth, uint64_t seed, uint32_t flags,
                                     const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void** d_out_bases,
                                     const void** d_out_offsets, const void** d_origin, const void** d_read_stats, const void** d_verdict,
                                     uint64_t* n_out, uint64_t* n_out_bases, uint64_t* summary) {
    if (n_out) *n_out = 0;
    if (n_out_bases) *n_out_bases = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_normalize_device";
    int rc;
    NormRule R;
    if ((rc = graph_begin(c, what, 0, 0)) || (rc = normalize_rule(c, what, permille, target, min_depth, seed, flags, n_reads, &R))) return rc;
    if (n_reads && (rc = check_device_batch(c, what, d_bases, d_offsets))) return rc;
    u64 h[KMC_NORMALIZE_WORDS];
    if ((rc = normalize_run(c, what, R, (const uint8_t*)d_bases, (const u64*)d_offsets, n_reads, n_reads ? n_bases : 0, h))) return rc;
    if (d_out_bases) *d_out_bases = c->nm_out.p;
    if (d_out_offsets) *d_out_offsets = c->nm_ooffs.p;
    if (d_origin) *d_origin = c->nm_origin.p;
    if (d_read_stats) *d_read_stats = c->nm_stats.p;
    if (d_verdict) *d_verdict = c->nm_verdict.p;
    if (n_out) *n_out = h[2];
    if (n_out_bases) *n_out_bases = h[3];
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

static int kmc_normalize_impl(kmc_ctx* c, uint32_t permille, uint64_t target, uint64_t min_depth, uint64_t seed, uint32_t flags,
                              const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint8_t* out_bases, uint64_t cap_bases,
                              uint64_t* out_offsets, uint64_t* origin, uint64_t cap_reads, uint32_t* read_stats, uint8_t* verdict, uint64_t* n_out,
                              uint64_t* n_out_bases, uint64_t* summary) {
    if (n_out) *n_out = 0;
    if (n_out_bases) *n_out_bases = 0;
    if (!c) return KMC_ERR_ARG;
    const char* what = "kmc_normalize";
    int rc;
    NormRule R;
    if ((rc = graph_begin(c, what, 0, 0)) || (rc = normalize_rule(c, what, permille, target, min_depth, seed, flags, n_reads, &R))) return rc;
    u64 n_bases = 0;
    if (n_reads && (rc = stage_batch(c, what, bases, offsets, n_reads, true, &n_bases))) return rc;
    u64 h[KMC_NORMALIZE_WORDS];
    if ((rc = normalize_run(c, what, R, (const uint8_t*)c->q_bases.p, (const u64*)c->q_offs.p, n_reads, n_bases, h))) return rc;
    const u64 no = h[2], nb = h[3];
    if (n_out) *n_out = no;
    if (n_out_bases) *n_out_bases = nb;
    if (out_bases && cap_bases < nb) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu bases", what, (unsigned long long)cap_bases, (unsigned long long)nb);
    if ((out_offsets || origin) && cap_reads < no) return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu reads", what, (unsigned long long)cap_reads, (unsigned long long)no);
    if (out_bases && nb) HIPCHK(c, hipMemcpyAsync(out_bases, c->nm_out.p, (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    if (out_offsets) HIPCHK(c, hipMemcpyAsync(out_offsets, c->nm_ooffs.p, (size_t)(no + 1) * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (origin && no) HIPCHK(c, hipMemcpyAsync(origin, c->nm_origin.p, (size_t)no * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (read_stats && n_reads) HIPCHK(c, hipMemcpyAsync(read_stats, c->nm_stats.p, (size_t)n_reads * KMC_NORMALIZE_READ_WORDS * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    if (verdict && n_reads) HIPCHK(c, hipMemcpyAsync(verdict, c->nm_verdict.p, (size_t)n_reads, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- the compacted graph cleaned: a verdict per unitig, the table of the kept keys (kmc_clean.hip.h) ----
static u64 clean_limit(uint64_t keys) { return keys >= (1ull << 31) ? ~0ull : (u64)keys; }   // 2^31 or more: unlimited

static bool clean_kept(const kmc_ctx* c, u64 min_count, u64 max_count, u64 tip, u64 isl, u64 bub) {
    return c->cl_key.holds(c->view_gen, min_count, max_count) && c->cl_tip == tip && c->cl_isl == isl && c->cl_bub == bub;
}

// The clean pass behind the unitigs and links of this view and range -- those the ctx holds if their work arrays are still
// theirs, otherwise computed and kept -- into cl_verdict / cl, the summary into cl_words; finished when it returns.
// bub != 0 runs the kernels that also pop bubbles; simplify says whose trace line the pass prints.
static int clean_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, u64 tip, u64 isl, u64 bub = 0, bool simplify = false) {
    int rc;
    u64 lw[KMC_LINK_WORDS];
    const bool held = c->u_live && c->u_key.holds(c->view_gen, min_count, max_count);
    if ((rc = links_result(c, what, min_count, max_count, held, lw))) return rc;
    c->cl_key.drop();
    const u64 n = c->n_sorted, nu = lw[0], nl = lw[1];
    u64 h[KMC_C_CTL_WORDS] = {0};
    if ((rc = ensure(c, c->cl_verdict, (size_t)std::max<u64>(nu, 8))) || (rc = ensure(c, c->cl_row, (size_t)std::max<u64>(n, 8)))) return rc;
    UnitigTrace tr;
    tr.mark(c->stream);
    if (nu) {
        if (nu > n || c->u_words[0] != nu) return fail(c, KMC_ERR_HIP, "internal error: %s holds %llu unitigs, its links %llu", what, (unsigned long long)c->u_words[0], (unsigned long long)nu);
        const u64 n_tiles = (n + KMC_C_TILE - 1) / KMC_C_TILE;
        if ((rc = compact_plan(c, n_tiles, KMC_C_CTL_WORDS))) return rc;
        kmc_ull* ctl = (kmc_ull*)c->c_ctl.p;
        CleanGraph g;
        g.offsets = (const u64*)c->u_offs.p; g.abund = (const u64*)c->u_abund.p; g.flags = (const uint8_t*)c->u_flags.p;
        g.link_offsets = (const u64*)c->l_offs.p; g.link_to = (const u32*)c->l_to.p;
        g.n_unitigs = nu; g.n_links = nl; g.km1 = (u64)(c->klen - 1); g.max_tip = tip; g.max_island = isl; g.max_bubble = bub;
        const u32 grid = (u32)std::min<u64>(n_tiles, (u64)c->n_cu * 8);
        if (bub && (rc = ensure(c, c->cl_part, (size_t)grid * KMC_C_PART * sizeof(u64)))) return rc;
        auto launch = [&](auto BUBBLES) {
            hipLaunchKernelGGL(kmc_clean_verdict_kernel<BUBBLES()>, dim3((u32)((nu + KMC_C_THREADS - 1) / KMC_C_THREADS)), dim3(KMC_C_THREADS), 0,
                               c->stream, g, (uint8_t*)c->cl_verdict.p, ctl);
            hipLaunchKernelGGL(kmc_clean_mark_kernel<BUBBLES()>, dim3(grid), dim3(KMC_C_THREADS), 0, c->stream, c->v_cnt, n, n_tiles,
                               (const uint16_t*)c->g_adj.p, (const u32*)c->u_ptr[c->u_cur].p, (const u32*)c->u_join.p, c->cfg.canonical ? 1 : 0,
                               (const uint8_t*)c->cl_verdict.p, nu, (uint8_t*)c->cl_row.p, (u32*)c->c_tile.p, ctl, (kmc_ull*)c->cl_part.p);
            if (BUBBLES())
                hipLaunchKernelGGL(kmc_clean_reduce_kernel, dim3(KMC_C_PART_USED), dim3(KMC_C_THREADS), 0, c->stream, (const kmc_ull*)c->cl_part.p, grid, ctl);
        };
        if (bub) launch(std::true_type{}); else launch(std::false_type{});
        if ((rc = compact_scan_and_read(c, n_tiles, h, KMC_C_CTL_WORDS))) return rc;
        if (h[KMC_C_BAD] || h[0] != h[KMC_C_SUM + 3] ||
            h[KMC_C_SUM + 3] + h[KMC_C_SUM + 4] + h[KMC_C_SUM + 5] + h[KMC_C_SUM2 + 1] != c->u_words[2])
            return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays (%llu + %llu + %llu + %llu of %llu keys, %llu scanned)",
                        what, (unsigned long long)h[KMC_C_BAD], (unsigned long long)h[KMC_C_SUM + 3], (unsigned long long)h[KMC_C_SUM + 4],
                        (unsigned long long)h[KMC_C_SUM + 5], (unsigned long long)h[KMC_C_SUM2 + 1], (unsigned long long)c->u_words[2],
                        (unsigned long long)h[0]);
    }
    const u64 n_kept = h[0];
    if ((rc = ensure_keys(c, c->cl, n_kept))) return rc;
    if (n_kept) {
        const KView v = view_of(c);
        const u64 n_tiles = (n + KMC_C_TILE - 1) / KMC_C_TILE;
        kmc_ull* ctl = (kmc_ull*)c->c_ctl.p;
        with_kw(c, [&](auto KW) {
            hipLaunchKernelGGL(kmc_clean_scatter_kernel<KW()>, dim3((u32)n_tiles), dim3(KMC_C_THREADS), 0, c->stream, v.hi, v.lo, v.cnt, v.n,
                               (const uint8_t*)c->cl_row.p, (const u32*)c->c_tpos.p, n_kept, (u64*)c->cl.hi.p, (u64*)c->cl.lo.p, (u64*)c->cl.cnt.p, ctl);
        });
        HIPCHK(c, hipGetLastError());
        u64 bad = 0;
        HIPCHK(c, hipMemcpyAsync(&bad, ctl + KMC_C_BAD, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, KMC_ERR_HIP, "internal error: %s could not place %llu kept keys", what, (unsigned long long)bad);
    }
    tr.mark(c->stream);
    if (tr.on && tr.n_ev == 2) {
        float ms = 0;
        if (hipEventSynchronize(tr.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, tr.ev[0], tr.ev[1]) == hipSuccess) {
            if (simplify)
                fprintf(stderr, "kmc_unitig_simplify: keys %llu unitigs %llu tips %llu islands %llu bubbles %llu kept %llu clean_ms %.4f\n",
                        (unsigned long long)n, (unsigned long long)nu, (unsigned long long)h[KMC_C_SUM + 1], (unsigned long long)h[KMC_C_SUM + 2],
                        (unsigned long long)h[KMC_C_SUM2 + 0], (unsigned long long)n_kept, ms);
            else
                fprintf(stderr, "kmc_unitig_clean: keys %llu unitigs %llu tips %llu islands %llu kept %llu clean_ms %.4f\n", (unsigned long long)n,
                        (unsigned long long)nu, (unsigned long long)h[KMC_C_SUM + 1], (unsigned long long)h[KMC_C_SUM + 2], (unsigned long long)n_kept, ms);
        }
    }
    h[KMC_C_SUM + 0] = nu;
    memcpy(c->cl_words, h + KMC_C_SUM, KMC_CLEAN_WORDS * sizeof(u64));
    memcpy(c->cl_words + KMC_CLEAN_WORDS, h + KMC_C_SUM2, (KMC_SIMPLIFY_WORDS - KMC_CLEAN_WORDS) * sizeof(u64));
    c->cl_kept = n_kept;
    c->cl_key.keep(c->view_gen, min_count, max_count); c->cl_tip = tip; c->cl_isl = isl; c->cl_bub = bub;
    return KMC_OK;
}

// what a clean and a simplify call differ in: the bubble limit, how many summary words go out, whose name errors carry
struct CleanForm { uint64_t max_bubble_keys; int words; bool simplify; const char* what; };

static int kmc_unitig_clean_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                                        const void** d_key_hi, const void** d_key_lo, const void** d_count, const void** d_verdict,
                                        uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary,
                                        CleanForm f = {0, KMC_CLEAN_WORDS, false, "kmc_unitig_clean_device"}) {
    if (!c) return KMC_ERR_ARG;
    int rc;
    const char* what = f.what;
    if ((rc = unitig_begin(c, what, min_count, max_count)) ||
        (rc = clean_run(c, what, min_count, max_count, clean_limit(max_tip_keys), clean_limit(max_island_keys), clean_limit(f.max_bubble_keys),
                        f.simplify))) return rc;
    publish_keys(c, c->cl, d_key_hi, d_key_lo, d_count);
    if (d_verdict) *d_verdict = c->cl_verdict.p;
    if (n_kept) *n_kept = c->cl_kept;
    if (n_unitigs) *n_unitigs = c->cl_words[0];
    if (summary) memcpy(summary, c->cl_words, (size_t)f.words * sizeof(u64));
    return KMC_OK;
}

static int kmc_unitig_clean_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                                 uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap_keys, uint8_t* verdict, uint64_t cap_unitigs,
                                 uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary,
                                 CleanForm f = {0, KMC_CLEAN_WORDS, false, "kmc_unitig_clean"}) {
    if (n_kept) *n_kept = 0;
    if (n_unitigs) *n_unitigs = 0;
    if (!c) return KMC_ERR_ARG;
    int rc;
    const char* what = f.what;
    if ((rc = unitig_begin(c, what, min_count, max_count))) return rc;
    const u64 tip = clean_limit(max_tip_keys), isl = clean_limit(max_island_keys), bub = clean_limit(f.max_bubble_keys);
    if (!clean_kept(c, min_count, max_count, tip, isl, bub) && (rc = clean_run(c, what, min_count, max_count, tip, isl, bub, f.simplify))) return rc;
    const u64 nk = c->cl_kept, nu = c->cl_words[0];
    if (n_kept) *n_kept = nk;
    if (n_unitigs) *n_unitigs = nu;
    if ((key_hi || key_lo || count) && cap_keys < nk)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu kept keys", what, (unsigned long long)cap_keys, (unsigned long long)nk);
    if (verdict && cap_unitigs < nu)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu unitigs", what, (unsigned long long)cap_unitigs, (unsigned long long)nu);
    if (nk && (rc = queue_to_host(c, c->cl.hi.p, c->cl.lo.p, c->cl.cnt.p, nk, key_hi, key_lo, count))) return rc;
    if (verdict && nu) HIPCHK(c, hipMemcpyAsync(verdict, c->cl_verdict.p, (size_t)nu, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, c->cl_words, (size_t)f.words * sizeof(u64));
    return KMC_OK;
}

// One step of a cleaning round: the kept pairs of src merged into dst's table (dst stays un-finalized).  dst's merge has
// finished when this returns: src's result may be rewritten right after.
static int kmc_unitig_clean_into_impl(kmc_ctx* src, kmc_ctx* dst, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys,
                                      uint64_t max_island_keys, uint64_t* summary,
                                      CleanForm f = {0, KMC_CLEAN_WORDS, false, "kmc_unitig_clean_into"}) {
    if (!src || !dst) return src ? fail(src, KMC_ERR_ARG, "%s: null context", f.what) : KMC_ERR_ARG;
    if (dst == src) return fail(src, KMC_ERR_ARG, "%s: dst is src", f.what);
    int rc;
    if ((rc = same_kind(src, dst, f.what))) return rc;
    const void *hi = nullptr, *lo = nullptr, *cnt = nullptr;
    uint64_t nk = 0;
    u64 h[KMC_SIMPLIFY_WORDS];
    if ((rc = kmc_unitig_clean_device_impl(src, min_count, max_count, max_tip_keys, max_island_keys, &hi, &lo, &cnt, nullptr, &nk, nullptr, h, f)))
        return rc;
    if (nk) {
        if ((rc = kmc_merge_pairs_device(dst, hi, lo, cnt, nk)) || (rc = kmc_sync(dst)))
            return fail(src, rc, "%s: merging into dst failed: %s", f.what, kmc_last_error(dst));
    }
    if (summary) memcpy(summary, h, (size_t)f.words * sizeof(u64));
    return KMC_OK;
}

// ---- the connected components of the compacted graph: a number per unitig, four words per component, the small ones
// dropped from the kept table (kmc_components.hip.h) ----
static bool components_kept(const kmc_ctx* c, u64 min_count, u64 max_count, u64 limit) {
    return c->cc_key.holds(c->view_gen, min_count, max_count) && c->cc_limit == limit;
}

// The label rounds on cc_parent (kmc_components.hip.h): batches of KMC_CC_ROUND_BATCH hook + shortcut rounds, their counters
// read in one copy, until a hook pass that hooked nothing.  A hook pass that hooks leaves a root fewer, so nu passes are the
// most there can be; beyond that the call fails.  *rounds: the passes up to and including the quiet one.
static int components_label(kmc_ctx* c, const char* what, u64 nu, u64 nl, u32* rounds) {
    u32* parent = (u32*)c->cc_parent.p;
    kmc_ull* ctl = (kmc_ull*)c->cc_ctl.p;
    kmc_ull* cnt = ctl + KMC_CC_ROUNDS_AT;
    const u32 grid_u = (u32)((nu + KMC_CC_THREADS - 1) / KMC_CC_THREADS);
    const u32 grid_e = (u32)std::min<u64>((2 * nu + KMC_CC_THREADS - 1) / KMC_CC_THREADS, (u64)c->n_cu * 4);
    hipLaunchKernelGGL(kmc_cc_init_kernel, dim3(grid_u), dim3(KMC_CC_THREADS), 0, c->stream, parent, nu);
    const u64 max_rounds = nu;
    u64 t = 0;
    bool done = false;
    while (!done && t < max_rounds) {
        const int batch = (int)std::min<u64>(KMC_CC_ROUND_BATCH, max_rounds - t);
        u64 h[KMC_CC_ROUND_BATCH] = {0};
        HIPCHK(c, hipMemsetAsync(cnt, 0, KMC_CC_ROUND_BATCH * sizeof(u64), c->stream));
        for (int i = 0; i < batch; ++i) {
            hipLaunchKernelGGL(kmc_cc_hook_kernel, dim3(grid_e), dim3(KMC_CC_THREADS), 0, c->stream, (const u64*)c->l_offs.p, (const u32*)c->l_to.p,
                               nu, nl, parent, cnt + i, ctl);
            hipLaunchKernelGGL(kmc_cc_shortcut_kernel, dim3(grid_u), dim3(KMC_CC_THREADS), 0, c->stream, parent, nu, ctl);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < batch && !done; ++i) { ++t; done = h[i] == 0; }
    }
    *rounds = (u32)std::min<u64>(t, 0xFFFFFFFFull);
    if (!done) return fail(c, KMC_ERR_HIP, "internal error: %s still hooked after %llu rounds over %llu unitigs", what, (unsigned long long)t, (unsigned long long)nu);
    return KMC_OK;
}

// The components pass behind the unitigs and links of this view and range -- those the ctx holds under clean_run's
// condition, otherwise computed and kept -- into the cc_* buffers, the summary into cc_words; finished when it returns.
// It shares the scratch of a compaction and the class bytes per row (cl_row) with the clean pass and writes nothing else of it.
static int components_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, u64 limit) {
    int rc;
    u64 lw[KMC_LINK_WORDS];
    const bool held = c->u_live && c->u_key.holds(c->view_gen, min_count, max_count);
    if ((rc = links_result(c, what, min_count, max_count, held, lw))) return rc;
    c->cc_key.drop();
    const u64 n = c->n_sorted, nu = lw[0], nl = lw[1];
    u64 w[KMC_CC_ROUNDS_AT] = {0}, h[KMC_C_CTL_WORDS] = {0}, nc = 0;
    u32 rounds = 0;
    if ((rc = ensure(c, c->cc_comp, (size_t)std::max<u64>(nu, 2) * sizeof(u32))) || (rc = ensure(c, c->cc_verdict, (size_t)std::max<u64>(nu, 8))) ||
        (rc = ensure(c, c->cc_stats, KMC_COMPONENT_STAT_WORDS * sizeof(u64))) || (rc = ensure(c, c->cl_row, (size_t)std::max<u64>(n, 8))))
        return rc;
    UnitigTrace tr;
    tr.mark(c->stream);
    if (nu) {
        if (nu > n || c->u_words[0] != nu) return fail(c, KMC_ERR_HIP, "internal error: %s holds %llu unitigs, its links %llu", what, (unsigned long long)c->u_words[0], (unsigned long long)nu);
        const size_t ub = (size_t)nu * sizeof(u32);
        if ((rc = ensure(c, c->cc_parent, ub)) || (rc = ensure(c, c->cc_flag, ub)) || (rc = ensure(c, c->cc_rank, ub)) ||
            (rc = ensure(c, c->cc_ctl, KMC_CC_CTL_BYTES)) ||
            (rc = ensure(c, c->c_bsum, (size_t)((nu + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK + 2) * sizeof(u32))))
            return rc;
        kmc_ull* ctl = (kmc_ull*)c->cc_ctl.p;
        HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_CC_CTL_BYTES, c->stream));
        if ((rc = components_label(c, what, nu, nl, &rounds))) return rc;
        tr.mark(c->stream);
        // number
        const u32 grid_u = (u32)((nu + KMC_CC_THREADS - 1) / KMC_CC_THREADS);
        hipLaunchKernelGGL(kmc_cc_flag_kernel, dim3(grid_u), dim3(KMC_CC_THREADS), 0, c->stream, (const u32*)c->cc_parent.p, nu, (u32*)c->cc_flag.p, ctl);
        launch_exclusive_scan<0>(c->stream, c->cc_flag.p, (u32)nu, (u32*)c->c_bsum.p, (u32*)c->cc_rank.p, (u32*)ctl);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nc = w[0] & 0xFFFFFFFFull;
        if (w[KMC_CC_BAD] || !nc || nc > nu)
            return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays (%llu components of %llu unitigs)", what,
                        (unsigned long long)w[KMC_CC_BAD], (unsigned long long)nc, (unsigned long long)nu);
        const size_t stb = (size_t)nc * KMC_COMPONENT_STAT_WORDS * sizeof(u64);
        const u32 grid_c = (u32)std::min<u64>((nc + KMC_CC_THREADS - 1) / KMC_CC_THREADS, (u64)c->n_cu * 8);
        if ((rc = ensure(c, c->cc_stats, stb)) || (rc = ensure(c, c->cc_part, (size_t)grid_c * KMC_CC_PART * sizeof(u64)))) return rc;
        kmc_ull* stats = (kmc_ull*)c->cc_stats.p;
        HIPCHK(c, hipMemsetAsync(stats, 0, stb, c->stream));
        hipLaunchKernelGGL(kmc_cc_number_kernel, dim3(grid_u), dim3(KMC_CC_THREADS), 0, c->stream, (const u32*)c->cc_parent.p, (const u32*)c->cc_rank.p,
                           nu, nc, (u32*)c->cc_comp.p, stats, ctl);
        HIPCHK(c, hipGetLastError());
        tr.mark(c->stream);
        // the words of every component, the verdicts, the summary
        hipLaunchKernelGGL(kmc_cc_stats_kernel, dim3(grid_u), dim3(KMC_CC_THREADS), 0, c->stream, (const u64*)c->u_offs.p, (const u64*)c->u_abund.p,
                           (u64)(c->klen - 1), (const u32*)c->cc_comp.p, nu, nc, stats, ctl);
        hipLaunchKernelGGL(kmc_cc_verdict_kernel, dim3(grid_u), dim3(KMC_CC_THREADS), 0, c->stream, (const u32*)c->cc_comp.p, (const kmc_ull*)stats, nu,
                           nc, limit, (uint8_t*)c->cc_verdict.p, ctl);
        hipLaunchKernelGGL(kmc_cc_summary_kernel, dim3(grid_c), dim3(KMC_CC_THREADS), 0, c->stream, (const kmc_ull*)stats, nc, limit, (kmc_ull*)c->cc_part.p);
        hipLaunchKernelGGL(kmc_cc_reduce_kernel, dim3(1), dim3(KMC_CC_THREADS), 0, c->stream, (const kmc_ull*)c->cc_part.p, grid_c, ctl);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        tr.mark(c->stream);
        if (w[KMC_CC_BAD] || w[KMC_CC_SMALLKEYS] > c->u_words[2])
            return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays (%llu keys in small components of %llu)", what,
                        (unsigned long long)w[KMC_CC_BAD], (unsigned long long)w[KMC_CC_SMALLKEYS], (unsigned long long)c->u_words[2]);
        // the kept table: the mark and scatter passes of the clean pass with this verdict array (any byte that is not KEEP
        // removes a row; their tip and island totals stay 0)
        const u64 n_tiles = (n + KMC_C_TILE - 1) / KMC_C_TILE;
        if ((rc = compact_plan(c, n_tiles, KMC_C_CTL_WORDS))) return rc;
        const u32 grid = (u32)std::min<u64>(n_tiles, (u64)c->n_cu * 8);
        hipLaunchKernelGGL(kmc_clean_mark_kernel<false>, dim3(grid), dim3(KMC_C_THREADS), 0, c->stream, c->v_cnt, n, n_tiles,
                           (const uint16_t*)c->g_adj.p, (const u32*)c->u_ptr[c->u_cur].p, (const u32*)c->u_join.p, c->cfg.canonical ? 1 : 0,
                           (const uint8_t*)c->cc_verdict.p, nu, (uint8_t*)c->cl_row.p, (u32*)c->c_tile.p, (kmc_ull*)c->c_ctl.p, (kmc_ull*)nullptr);
        if ((rc = compact_scan_and_read(c, n_tiles, h, KMC_C_CTL_WORDS))) return rc;
        if (h[KMC_C_BAD] || h[0] != h[KMC_C_SUM + 3] || h[KMC_C_SUM + 4] || h[KMC_C_SUM + 5] || h[KMC_C_SUM + 3] + w[KMC_CC_SMALLKEYS] != c->u_words[2])
            return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays (%llu kept + %llu small of %llu keys, %llu scanned)",
                        what, (unsigned long long)h[KMC_C_BAD], (unsigned long long)h[KMC_C_SUM + 3], (unsigned long long)w[KMC_CC_SMALLKEYS],
                        (unsigned long long)c->u_words[2], (unsigned long long)h[0]);
    }
    const u64 n_kept = h[0];
    if ((rc = ensure_keys(c, c->cc, n_kept))) return rc;
    if (n_kept) {
        const KView v = view_of(c);
        const u64 n_tiles = (n + KMC_C_TILE - 1) / KMC_C_TILE;
        kmc_ull* ctl = (kmc_ull*)c->c_ctl.p;
        with_kw(c, [&](auto KW) {
            hipLaunchKernelGGL(kmc_clean_scatter_kernel<KW()>, dim3((u32)n_tiles), dim3(KMC_C_THREADS), 0, c->stream, v.hi, v.lo, v.cnt, v.n,
                               (const uint8_t*)c->cl_row.p, (const u32*)c->c_tpos.p, n_kept, (u64*)c->cc.hi.p, (u64*)c->cc.lo.p, (u64*)c->cc.cnt.p, ctl);
        });
        HIPCHK(c, hipGetLastError());
        u64 bad = 0;
        HIPCHK(c, hipMemcpyAsync(&bad, ctl + KMC_C_BAD, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, KMC_ERR_HIP, "internal error: %s could not place %llu kept keys", what, (unsigned long long)bad);
    }
    tr.mark(c->stream);
    if (tr.on && nu && tr.n_ev == 5) {
        float ms[4] = {0, 0, 0, 0};
        bool ok = hipEventSynchronize(tr.ev[4]) == hipSuccess;
        for (int i = 0; ok && i < 4; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_unitig_components: keys %llu unitigs %llu records %llu components %llu small %llu kept %llu rounds %u "
                    "label_ms %.4f number_ms %.4f stats_ms %.4f keep_ms %.4f\n", (unsigned long long)n, (unsigned long long)nu, (unsigned long long)nl,
                    (unsigned long long)nc, (unsigned long long)w[KMC_CC_SMALL], (unsigned long long)n_kept, rounds, ms[0], ms[1], ms[2], ms[3]);
    }
    u64* s = c->cc_words;
    s[0] = nu; s[1] = nc; s[2] = w[KMC_CC_SINGLE]; s[3] = w[KMC_CC_MAXKEYS]; s[4] = w[KMC_CC_MAXUNI]; s[5] = w[KMC_CC_SMALL];
    s[6] = n_kept; s[7] = h[KMC_C_SUM + 7];
    c->cc_kept = n_kept; c->cc_comps = nc;
    c->cc_key.keep(c->view_gen, min_count, max_count); c->cc_limit = limit;
    return KMC_OK;
}

static int kmc_unitig_components_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_component_keys,
                                             const void** d_comp_of, const void** d_comp_stats, const void** d_verdict, const void** d_key_hi,
                                             const void** d_key_lo, const void** d_count, uint64_t* n_comps, uint64_t* n_unitigs, uint64_t* n_kept,
                                             uint64_t* summary, const char* what = "kmc_unitig_components_device") {
    if (!c) return KMC_ERR_ARG;
    int rc;
    if ((rc = unitig_begin(c, what, min_count, max_count)) || (rc = components_run(c, what, min_count, max_count, clean_limit(max_component_keys))))
        return rc;
    publish_keys(c, c->cc, d_key_hi, d_key_lo, d_count);
    if (d_comp_of) *d_comp_of = c->cc_comp.p;
    if (d_comp_stats) *d_comp_stats = c->cc_stats.p;
    if (d_verdict) *d_verdict = c->cc_verdict.p;
    if (n_comps) *n_comps = c->cc_comps;
    if (n_unitigs) *n_unitigs = c->cc_words[0];
    if (n_kept) *n_kept = c->cc_kept;
    if (summary) memcpy(summary, c->cc_words, sizeof(c->cc_words));
    return KMC_OK;
}

static int kmc_unitig_components_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_component_keys, uint32_t* comp_of,
                                      uint8_t* verdict, uint64_t cap_unitigs, uint64_t* comp_stats, uint64_t cap_comps, uint64_t* key_hi,
                                      uint64_t* key_lo, uint64_t* count, uint64_t cap_keys, uint64_t* n_comps, uint64_t* n_unitigs, uint64_t* n_kept,
                                      uint64_t* summary) {
    if (n_comps) *n_comps = 0;
    if (n_unitigs) *n_unitigs = 0;
    if (n_kept) *n_kept = 0;
    if (!c) return KMC_ERR_ARG;
    int rc;
    const char* what = "kmc_unitig_components";
    if ((rc = unitig_begin(c, what, min_count, max_count))) return rc;
    const u64 limit = clean_limit(max_component_keys);
    if (!components_kept(c, min_count, max_count, limit) && (rc = components_run(c, what, min_count, max_count, limit))) return rc;
    const u64 nk = c->cc_kept, nu = c->cc_words[0], nc = c->cc_comps;
    if (n_comps) *n_comps = nc;
    if (n_unitigs) *n_unitigs = nu;
    if (n_kept) *n_kept = nk;
    if ((key_hi || key_lo || count) && cap_keys < nk)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu kept keys", what, (unsigned long long)cap_keys, (unsigned long long)nk);
    if ((comp_of || verdict) && cap_unitigs < nu)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu unitigs", what, (unsigned long long)cap_unitigs, (unsigned long long)nu);
    if (comp_stats && cap_comps < nc)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu components", what, (unsigned long long)cap_comps, (unsigned long long)nc);
    if (nk && (rc = queue_to_host(c, c->cc.hi.p, c->cc.lo.p, c->cc.cnt.p, nk, key_hi, key_lo, count))) return rc;
    if (comp_of && nu) HIPCHK(c, hipMemcpyAsync(comp_of, c->cc_comp.p, (size_t)nu * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    if (verdict && nu) HIPCHK(c, hipMemcpyAsync(verdict, c->cc_verdict.p, (size_t)nu, hipMemcpyDeviceToHost, c->stream));
    if (comp_stats && nc)
        HIPCHK(c, hipMemcpyAsync(comp_stats, c->cc_stats.p, (size_t)nc * KMC_COMPONENT_STAT_WORDS * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, c->cc_words, sizeof(c->cc_words));
    return KMC_OK;
}

// One step of a round that drops small components: the kept pairs of src merged into dst's table, as kmc_unitig_clean_into.
static int kmc_unitig_components_into_impl(kmc_ctx* src, kmc_ctx* dst, uint64_t min_count, uint64_t max_count, uint64_t max_component_keys,
                                           uint64_t* summary) {
    const char* what = "kmc_unitig_components_into";
    if (!src || !dst) return src ? fail(src, KMC_ERR_ARG, "%s: null context", what) : KMC_ERR_ARG;
    if (dst == src) return fail(src, KMC_ERR_ARG, "%s: dst is src", what);
    int rc;
    if ((rc = same_kind(src, dst, what))) return rc;
    const void *hi = nullptr, *lo = nullptr, *cnt = nullptr;
    uint64_t nk = 0;
    u64 h[KMC_COMPONENT_WORDS];
    if ((rc = kmc_unitig_components_device_impl(src, min_count, max_count, max_component_keys, nullptr, nullptr, nullptr, &hi, &lo, &cnt, nullptr,
                                                nullptr, &nk, h, what)))
        return rc;
    if (nk) {
        if ((rc = kmc_merge_pairs_device(dst, hi, lo, cnt, nk)) || (rc = kmc_sync(dst)))
            return fail(src, rc, "%s: merging into dst failed: %s", what, kmc_last_error(dst));
    }
    if (summary) memcpy(summary, h, sizeof(h));
    return KMC_OK;
}

// ---- the bubbles of the compacted graph as variant records: eight words per called arm (kmc_bubbles.hip.h) ----
static bool bubbles_kept(const kmc_ctx* c, u64 min_count, u64 max_count, u64 limit) {
    return c->bb_key.holds(c->view_gen, min_count, max_count) && c->bb_limit == limit;
}

// the limit of a bubbles call: unlike a clean limit it has no "unlimited" (a record's positions are u32)
static int bubbles_limit(kmc_ctx* c, const char* what, uint64_t max_bubble_keys) {
    if (max_bubble_keys >= (1ull << 31))
        return fail(c, KMC_ERR_ARG, "%s: max_bubble_keys %llu is 2^31 or more (a record's positions are 32-bit)", what, (unsigned long long)max_bubble_keys);
    return KMC_OK;
}

// The bubbles pass behind the unitigs and links of this view and range -- those the ctx holds under clean_run's condition,
// otherwise computed and kept -- into bb_rec, the summary into bb_words; finished when it returns.  It shares the block sums
// of a scan (c_bsum) with the other passes and writes nothing else of theirs.
static int bubbles_run(kmc_ctx* c, const char* what, u64 min_count, u64 max_count, u64 limit) {
    int rc;
    u64 lw[KMC_LINK_WORDS];
    const bool held = c->u_live && c->u_key.holds(c->view_gen, min_count, max_count);
    if ((rc = links_result(c, what, min_count, max_count, held, lw))) return rc;
    c->bb_key.drop();
    const u64 n = c->n_sorted, nu = lw[0], nl = lw[1];
    u64 w[KMC_B_CTL_WORDS] = {0}, nr = 0;
    if ((rc = ensure(c, c->bb_rec, KMC_B_REC * sizeof(u32)))) return rc;
    CleanGraph g;   // (read once the links stand: the unitig and link arrays, the candidate limit)
    g.offsets = (const u64*)c->u_offs.p; g.abund = (const u64*)c->u_abund.p; g.flags = (const uint8_t*)c->u_flags.p;
    g.link_offsets = (const u64*)c->l_offs.p; g.link_to = (const u32*)c->l_to.p;
    g.n_unitigs = nu; g.n_links = nl; g.km1 = (u64)(c->klen - 1); g.max_tip = 0; g.max_island = 0; g.max_bubble = limit;
    const u32 grid_u = (u32)((nu + KMC_B_THREADS - 1) / KMC_B_THREADS);
    UnitigTrace tr;
    tr.mark(c->stream);
    if (nu && limit) {
        if (nu > n || c->u_words[0] != nu) return fail(c, KMC_ERR_HIP, "internal error: %s holds %llu unitigs, its links %llu", what, (unsigned long long)c->u_words[0], (unsigned long long)nu);
        const size_t ub = (size_t)nu * sizeof(u32);
        if ((rc = ensure(c, c->bb_flag, ub)) || (rc = ensure(c, c->bb_pos, ub)) || (rc = ensure(c, c->bb_major, ub)) ||
            (rc = ensure(c, c->bb_ctl, KMC_B_CTL_WORDS * sizeof(u64))) ||
            (rc = ensure(c, c->c_bsum, (size_t)((nu + KMC_SCAN_PER_BLOCK - 1) / KMC_SCAN_PER_BLOCK + 2) * sizeof(u32))))
            return rc;
        kmc_ull* ctl = (kmc_ull*)c->bb_ctl.p;
        HIPCHK(c, hipMemsetAsync(ctl, 0, KMC_B_CTL_WORDS * sizeof(u64), c->stream));
        hipLaunchKernelGGL(kmc_bubble_pair_kernel, dim3(grid_u), dim3(KMC_B_THREADS), 0, c->stream, g, (u32*)c->bb_flag.p, (u32*)c->bb_major.p, ctl);
        launch_exclusive_scan<0>(c->stream, c->bb_flag.p, (u32)nu, (u32*)c->c_bsum.p, (u32*)c->bb_pos.p, (u32*)ctl);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nr = w[0] & 0xFFFFFFFFull;
        if (w[KMC_B_BAD] || nr != w[KMC_B_CALLED] || nr > w[KMC_B_CAND] || w[KMC_B_CAND] > nu)
            return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays (%llu called, %llu scanned, %llu candidates of %llu unitigs)",
                        what, (unsigned long long)w[KMC_B_BAD], (unsigned long long)w[KMC_B_CALLED], (unsigned long long)nr,
                        (unsigned long long)w[KMC_B_CAND], (unsigned long long)nu);
    }
    tr.mark(c->stream);
    if (nr) {
        if ((rc = ensure(c, c->bb_rec, (size_t)nr * KMC_B_REC * sizeof(u32)))) return rc;
        kmc_ull* ctl = (kmc_ull*)c->bb_ctl.p;
        const u32 grid_r = (u32)std::min<u64>((nr + KMC_B_WAVES - 1) / KMC_B_WAVES, (u64)c->n_cu * 8);
        hipLaunchKernelGGL(kmc_bubble_place_kernel, dim3(grid_u), dim3(KMC_B_THREADS), 0, c->stream, g, (const u32*)c->bb_flag.p, (const u32*)c->bb_pos.p,
                           (const u32*)c->bb_major.p, nr, (u32*)c->bb_rec.p, ctl);
        hipLaunchKernelGGL(kmc_bubble_diff_kernel, dim3(grid_r), dim3(KMC_B_THREADS), 0, c->stream, g, (const uint8_t*)c->u_bases.p, c->u_words[1], nr,
                           (u32*)c->bb_rec.p, ctl);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (w[KMC_B_BAD] || w[KMC_B_SUBST] + w[KMC_B_INDEL] + w[KMC_B_COMPLEX] != nr)
            return fail(c, KMC_ERR_HIP, "internal error: %s met %llu indices outside their arrays (%llu + %llu + %llu of %llu records)", what,
                        (unsigned long long)w[KMC_B_BAD], (unsigned long long)w[KMC_B_SUBST], (unsigned long long)w[KMC_B_INDEL],
                        (unsigned long long)w[KMC_B_COMPLEX], (unsigned long long)nr);
    }
    tr.mark(c->stream);
    if (tr.on && tr.n_ev == 3) {
        float ms[2] = {0, 0};
        bool ok = hipEventSynchronize(tr.ev[2]) == hipSuccess;
        for (int i = 0; ok && i < 2; ++i) ok = hipEventElapsedTime(&ms[i], tr.ev[i], tr.ev[i + 1]) == hipSuccess;
        if (ok)
            fprintf(stderr, "kmc_unitig_bubbles: keys %llu unitigs %llu candidates %llu records %llu subst %llu indel %llu complex %llu reversed %llu "
                    "pair_ms %.4f diff_ms %.4f\n", (unsigned long long)n, (unsigned long long)nu, (unsigned long long)w[KMC_B_CAND], (unsigned long long)nr,
                    (unsigned long long)w[KMC_B_SUBST], (unsigned long long)w[KMC_B_INDEL], (unsigned long long)w[KMC_B_COMPLEX],
                    (unsigned long long)w[KMC_B_REVERSED], ms[0], ms[1]);
    }
    u64* s = c->bb_words;
    s[0] = nu; s[1] = nr; s[2] = w[KMC_B_CAND]; s[3] = w[KMC_B_SUBST]; s[4] = w[KMC_B_INDEL]; s[5] = w[KMC_B_COMPLEX]; s[6] = w[KMC_B_REVERSED];
    s[7] = w[KMC_B_KEYS];
    c->bb_records = nr;
    c->bb_key.keep(c->view_gen, min_count, max_count); c->bb_limit = limit;
    return KMC_OK;
}

static int kmc_unitig_bubbles_device_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_bubble_keys, const void** d_records,
                                          uint64_t* n_records, uint64_t* n_unitigs, uint64_t* summary) {
    if (!c) return KMC_ERR_ARG;
    int rc;
    const char* what = "kmc_unitig_bubbles_device";
    if ((rc = unitig_begin(c, what, min_count, max_count)) || (rc = bubbles_limit(c, what, max_bubble_keys)) ||
        (rc = bubbles_run(c, what, min_count, max_count, (u64)max_bubble_keys))) return rc;
    if (d_records) *d_records = c->bb_rec.p;
    if (n_records) *n_records = c->bb_records;
    if (n_unitigs) *n_unitigs = c->bb_words[0];
    if (summary) memcpy(summary, c->bb_words, sizeof(c->bb_words));
    return KMC_OK;
}

static int kmc_unitig_bubbles_impl(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_bubble_keys, uint32_t* records,
                                   uint64_t cap_records, uint64_t* n_records, uint64_t* n_unitigs, uint64_t* summary) {
    if (n_records) *n_records = 0;
    if (n_unitigs) *n_unitigs = 0;
    if (!c) return KMC_ERR_ARG;
    int rc;
    const char* what = "kmc_unitig_bubbles";
    if ((rc = unitig_begin(c, what, min_count, max_count)) || (rc = bubbles_limit(c, what, max_bubble_keys))) return rc;
    const u64 limit = (u64)max_bubble_keys;
    if (!bubbles_kept(c, min_count, max_count, limit) && (rc = bubbles_run(c, what, min_count, max_count, limit))) return rc;
    const u64 nr = c->bb_records;
    if (n_records) *n_records = nr;
    if (n_unitigs) *n_unitigs = c->bb_words[0];
    if (records && cap_records < nr)
        return fail(c, KMC_ERR_ARG, "%s: capacity %llu < %llu records", what, (unsigned long long)cap_records, (unsigned long long)nr);
    if (records && nr) HIPCHK(c, hipMemcpyAsync(records, c->bb_rec.p, (size_t)nr * KMC_B_REC * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (summary) memcpy(summary, c->bb_words, sizeof(c->bb_words));
    return KMC_OK;
}

// ---- the ABI proper (guarded: no C++ exception leaves the library) ----
extern "C" int kmc_export(kmc_ctx* c, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap) {
    return guarded(c, [&]() -> int { return kmc_export_impl(c, key_hi, key_lo, count, cap); });
}
extern "C" int kmc_export_device(kmc_ctx* c, const void** d_key_hi, const void** d_key_lo, const void** d_count, uint64_t* n_distinct) {
    return guarded(c, [&]() -> int { return kmc_export_device_impl(c, d_key_hi, d_key_lo, d_count, n_distinct); });
}
extern "C" int kmc_histogram(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint32_t n_bins, uint64_t* hist, uint64_t* max_seen) {
    return guarded(c, [&]() -> int { return kmc_histogram_impl(c, min_count, max_count, n_bins, hist, max_seen); });
}
extern "C" int kmc_filter_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void** d_key_hi, const void** d_key_lo,
                                 const void** d_count, uint64_t* n_kept, uint64_t* kept_total) {
    return guarded(c, [&]() -> int { return kmc_filter_device_impl(c, min_count, max_count, d_key_hi, d_key_lo, d_count, n_kept, kept_total); });
}
extern "C" int kmc_export_filtered(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t* key_hi, uint64_t* key_lo,
                                   uint64_t* count, uint64_t cap, uint64_t* n_kept) {
    return guarded(c, [&]() -> int { return kmc_export_filtered_impl(c, min_count, max_count, key_hi, key_lo, count, cap, n_kept); });
}
extern "C" int kmc_query(kmc_ctx* c, const uint64_t* key_hi, const uint64_t* key_lo, uint64_t n_keys, uint64_t* count) {
    return guarded(c, [&]() -> int { return kmc_query_impl(c, key_hi, key_lo, n_keys, count); });
}
extern "C" int kmc_query_device(kmc_ctx* c, const void* d_key_hi, const void* d_key_lo, uint64_t n_keys, void* d_count) {
    return guarded(c, [&]() -> int { return kmc_query_device_impl(c, d_key_hi, d_key_lo, n_keys, d_count); });
}
extern "C" int kmc_profile(kmc_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t min_count,
                           uint32_t* window_count, uint64_t* read_stats) {
    return guarded(c, [&]() -> int { return kmc_profile_impl(c, bases, offsets, n_reads, min_count, window_count, read_stats); });
}
extern "C" int kmc_profile_device(kmc_ctx* c, const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
                                  uint64_t min_count, void* d_window_count, void* d_read_stats) {
    return guarded(c, [&]() -> int { return kmc_profile_device_impl(c, d_bases, d_offsets, n_reads, n_bases, min_count, d_window_count, d_read_stats); });
}
extern "C" int kmc_compare(kmc_ctx* a, kmc_ctx* b, uint64_t min_a, uint64_t max_a, uint64_t min_b, uint64_t max_b, uint64_t* summary) {
    return guarded(a, [&]() -> int { return kmc_compare_impl(a, b, min_a, max_a, min_b, max_b, summary); });
}
extern "C" int kmc_setop_device(kmc_ctx* a, kmc_ctx* b, int op, int count_mode, uint64_t min_a, uint64_t max_a, uint64_t min_b,
                                uint64_t max_b, const void** d_key_hi, const void** d_key_lo, const void** d_count, uint64_t* n_out,
                                uint64_t* total_out, uint64_t* summary) {
    return guarded(a, [&]() -> int {
        return kmc_setop_device_impl(a, b, op, count_mode, min_a, max_a, min_b, max_b, d_key_hi, d_key_lo, d_count, n_out, total_out, summary);
    });
}
extern "C" int kmc_export_setop(kmc_ctx* a, kmc_ctx* b, int op, int count_mode, uint64_t min_a, uint64_t max_a, uint64_t min_b,
                                uint64_t max_b, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap, uint64_t* n_out) {
    return guarded(a, [&]() -> int {
        return kmc_export_setop_impl(a, b, op, count_mode, min_a, max_a, min_b, max_b, key_hi, key_lo, count, cap, n_out);
    });
}
extern "C" int kmc_graph_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void** d_adj, uint64_t* n_keys, uint64_t* summary) {
    return guarded(c, [&]() -> int { return kmc_graph_device_impl(c, min_count, max_count, d_adj, n_keys, summary); });
}
extern "C" int kmc_graph(kmc_ctx* c, uint64_t min_count, uint64_t max_count, void* adj, uint64_t cap, uint64_t* n_keys, uint64_t* summary) {
    return guarded(c, [&]() -> int { return kmc_graph_impl(c, min_count, max_count, adj, cap, n_keys, summary); });
}
extern "C" int kmc_unitigs_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void** d_bases, const void** d_offsets,
                                  const void** d_abund, const void** d_flags, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitigs_device_impl(c, min_count, max_count, d_bases, d_offsets, d_abund, d_flags, n_unitigs, n_bases, summary);
    });
}
extern "C" int kmc_unitigs(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint8_t* bases, uint64_t cap_bases, uint64_t* offsets,
                           uint64_t* abund, uint8_t* flags, uint64_t cap_unitigs, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitigs_impl(c, min_count, max_count, bases, cap_bases, offsets, abund, flags, cap_unitigs, n_unitigs, n_bases, summary);
    });
}
extern "C" int kmc_unitig_links_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void** d_link_offsets, const void** d_link_to,
                                       uint64_t* n_unitigs, uint64_t* n_links, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_links_device_impl(c, min_count, max_count, d_link_offsets, d_link_to, n_unitigs, n_links, summary);
    });
}
extern "C" int kmc_unitig_links(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t* link_offsets, uint64_t cap_ends,
                                uint32_t* link_to, uint64_t cap_links, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_links_impl(c, min_count, max_count, link_offsets, cap_ends, link_to, cap_links, n_unitigs, n_links, summary);
    });
}
extern "C" int kmc_unitig_map_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void* d_bases, const void* d_offsets, uint64_t n_reads,
                                     uint64_t n_bases, const void** d_place, const void** d_read_stats, const void** d_seg_offsets,
                                     const void** d_segs, const void** d_support, uint64_t* n_segs, uint64_t* n_unitigs, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_map_device_impl(c, min_count, max_count, d_bases, d_offsets, n_reads, n_bases, d_place, d_read_stats, d_seg_offsets,
                                          d_segs, d_support, n_segs, n_unitigs, summary);
    });
}
extern "C" int kmc_unitig_map(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                              uint64_t* place, uint32_t* read_stats, uint64_t* seg_offsets, uint32_t* segs, uint64_t cap_segs,
                              uint64_t* support, uint64_t cap_unitigs, uint64_t* n_segs, uint64_t* n_unitigs, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_map_impl(c, min_count, max_count, bases, offsets, n_reads, place, read_stats, seg_offsets, segs, cap_segs, support,
                                   cap_unitigs, n_segs, n_unitigs, summary);
    });
}
extern "C" int kmc_unitig_transits_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint32_t flags, const void* d_bases,
                                          const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void** d_link_support,
                                          const void** d_transit_offsets, const void** d_transit_count, const void** d_verdict, uint64_t* n_unitigs,
                                          uint64_t* n_links, uint64_t* n_slots, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_transits_device_impl(c, min_count, max_count, min_reads, flags, d_bases, d_offsets, n_reads, n_bases, d_link_support,
                                               d_transit_offsets, d_transit_count, d_verdict, n_unitigs, n_links, n_slots, summary);
    });
}
extern "C" int kmc_unitig_pairs_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t n_bins, uint32_t flags, const void* d_bases,
                                       const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void** d_pair_class, const void** d_pair_ends,
                                       const void** d_pair_value, const void** d_rec_ends, const void** d_rec_count, const void** d_rec_sum,
                                       const void** d_rec_min, const void** d_rec_max, const void** d_insert_hist, uint64_t* n_pairs,
                                       uint64_t* n_records, uint64_t* summary) {
    return guarded(c, [&] {
        return kmc_unitig_pairs_device_impl(c, min_count, max_count, n_bins, flags, d_bases, d_offsets, n_reads, n_bases, d_pair_class, d_pair_ends,
                                            d_pair_value, d_rec_ends, d_rec_count, d_rec_sum, d_rec_min, d_rec_max, d_insert_hist, n_pairs, n_records, summary);
    });
}
extern "C" int kmc_unitig_pairs(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t n_bins, uint32_t flags, const uint8_t* bases,
                                const uint64_t* offsets, uint64_t n_reads, uint8_t* pair_class, uint32_t* pair_ends, uint64_t* pair_value,
                                uint64_t cap_pairs, uint32_t* rec_ends, uint64_t* rec_count, uint64_t* rec_sum, uint64_t* rec_min, uint64_t* rec_max,
                                uint64_t cap_records, uint64_t* insert_hist, uint64_t cap_bins, uint64_t* n_pairs, uint64_t* n_records,
                                uint64_t* summary) {
    return guarded(c, [&] {
        return kmc_unitig_pairs_impl(c, min_count, max_count, n_bins, flags, bases, offsets, n_reads, pair_class, pair_ends, pair_value, cap_pairs,
                                     rec_ends, rec_count, rec_sum, rec_min, rec_max, cap_records, insert_hist, cap_bins, n_pairs, n_records, summary);
    });
}
extern "C" int kmc_unitig_transits(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint32_t flags, const uint8_t* bases,
                                   const uint64_t* offsets, uint64_t n_reads, uint64_t* link_support, uint64_t cap_links, uint64_t* transit_offsets,
                                   uint64_t cap_unitigs, uint64_t* transit_count, uint64_t cap_slots, uint8_t* verdict, uint64_t* n_unitigs,
                                   uint64_t* n_links, uint64_t* n_slots, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_transits_impl(c, min_count, max_count, min_reads, flags, bases, offsets, n_reads, link_support, cap_links, transit_offsets,
                                        cap_unitigs, transit_count, cap_slots, verdict, n_unitigs, n_links, n_slots, summary);
    });
}
extern "C" int kmc_unitig_contigs_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint64_t min_support,
                                         const void** d_bases, const void** d_offsets, const void** d_path_offsets, const void** d_path,
                                         const void** d_abund, const void** d_flags, uint64_t* n_contigs, uint64_t* n_nodes, uint64_t* n_bases,
                                         uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_contigs_device_impl(c, min_count, max_count, min_reads, min_support, d_bases, d_offsets, d_path_offsets, d_path, d_abund,
                                              d_flags, n_contigs, n_nodes, n_bases, summary);
    });
}
extern "C" int kmc_unitig_contigs(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint64_t min_support, uint8_t* bases,
                                  uint64_t cap_bases, uint64_t* offsets, uint64_t* path_offsets, uint64_t* abund, uint8_t* flags,
                                  uint64_t cap_contigs, uint32_t* path, uint64_t cap_nodes, uint64_t* n_contigs, uint64_t* n_nodes,
                                  uint64_t* n_bases, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_contigs_impl(c, min_count, max_count, min_reads, min_support, bases, cap_bases, offsets, path_offsets, abund, flags,
                                       cap_contigs, path, cap_nodes, n_contigs, n_nodes, n_bases, summary);
    });
}
extern "C" int kmc_correct_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const void* d_bases, const void* d_offsets, uint64_t n_reads,
                                  uint64_t n_bases, const void** d_corrected, const void** d_read_stats, const void** d_cand_offsets,
                                  const void** d_cands, uint64_t* n_cands, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_correct_device_impl(c, min_count, max_count, d_bases, d_offsets, n_reads, n_bases, d_corrected, d_read_stats, d_cand_offsets, d_cands,
                                       n_cands, summary);
    });
}
extern "C" int kmc_correct(kmc_ctx* c, uint64_t min_count, uint64_t max_count, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
                           uint8_t* out_bases, uint32_t* read_stats, uint64_t* cand_offsets, uint32_t* cands, uint64_t cap_cands, uint64_t* n_cands,
                           uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_correct_impl(c, min_count, max_count, bases, offsets, n_reads, out_bases, read_stats, cand_offsets, cands, cap_cands, n_cands, summary);
    });
}
extern "C" int kmc_trim_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, int mode, uint32_t flags, uint64_t min_strong, uint32_t min_permille,
                               uint64_t min_len, const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
                               const void** d_out_bases, const void** d_out_offsets, const void** d_origin, const void** d_read_stats,
                               const void** d_verdict, uint64_t* n_out, uint64_t* n_out_bases, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_trim_device_impl(c, min_count, max_count, mode, flags, min_strong, min_permille, min_len, d_bases, d_offsets, n_reads, n_bases,
                                    d_out_bases, d_out_offsets, d_origin, d_read_stats, d_verdict, n_out, n_out_bases, summary);
    });
}
extern "C" int kmc_trim(kmc_ctx* c, uint64_t min_count, uint64_t max_count, int mode, uint32_t flags, uint64_t min_strong, uint32_t min_permille,
                        uint64_t min_len, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint8_t* out_bases, uint64_t cap_bases,
                        uint64_t* out_offsets, uint64_t* origin, uint64_t cap_reads, uint32_t* read_stats, uint8_t* verdict, uint64_t* n_out,
                        uint64_t* n_out_bases, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_trim_impl(c, min_count, max_count, mode, flags, min_strong, min_permille, min_len, bases, offsets, n_reads, out_bases, cap_bases,
                             out_offsets, origin, cap_reads, read_stats, verdict, n_out, n_out_bases, summary);
    });
}
extern "C" int kmc_normalize_device(kmc_ctx* c, uint32_t permille, uint64_t target, uint64_t min_depth, uint64_t seed, uint32_t flags,
                                    const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void** d_out_bases,
                                    const void** d_out_offsets, const void** d_origin, const void** d_read_stats, const void** d_verdict,
                                    uint64_t* n_out, uint64_t* n_out_bases, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_normalize_device_impl(c, permille, target, min_depth, seed, flags, d_bases, d_offsets, n_reads, n_bases, d_out_bases, d_out_offsets,
                                         d_origin, d_read_stats, d_verdict, n_out, n_out_bases, summary);
    });
}
extern "C" int kmc_normalize(kmc_ctx* c, uint32_t permille, uint64_t target, uint64_t min_depth, uint64_t seed, uint32_t flags, const uint8_t* bases,
                             const uint64_t* offsets, uint64_t n_reads, uint8_t* out_bases, uint64_t cap_bases, uint64_t* out_offsets,
                             uint64_t* origin, uint64_t cap_reads, uint32_t* read_stats, uint8_t* verdict, uint64_t* n_out, uint64_t* n_out_bases,
                             uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_normalize_impl(c, permille, target, min_depth, seed, flags, bases, offsets, n_reads, out_bases, cap_bases, out_offsets, origin,
                                  cap_reads, read_stats, verdict, n_out, n_out_bases, summary);
    });
}
extern "C" int kmc_unitig_clean_device(kmc_ctx* c,uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                                       const void** d_key_hi, const void** d_key_lo, const void** d_count, const void** d_verdict,
                                       uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_clean_device_impl(c, min_count, max_count, max_tip_keys, max_island_keys, d_key_hi, d_key_lo, d_count, d_verdict, n_kept,
                                            n_unitigs, summary);
    });
}
extern "C" int kmc_unitig_clean(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                                uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap_keys, uint8_t* verdict, uint64_t cap_unitigs,
                                uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_clean_impl(c, min_count, max_count, max_tip_keys, max_island_keys, key_hi, key_lo, count, cap_keys, verdict, cap_unitigs,
                                     n_kept, n_unitigs, summary);
    });
}
extern "C" int kmc_unitig_clean_into(kmc_ctx* src, kmc_ctx* dst, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys,
                                     uint64_t max_island_keys, uint64_t* summary) {
    return guarded(src, [&]() -> int {
        return kmc_unitig_clean_into_impl(src, dst, min_count, max_count, max_tip_keys, max_island_keys, summary);
    });
}
extern "C" int kmc_unitig_simplify_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                                          uint64_t max_bubble_keys, const void** d_key_hi, const void** d_key_lo, const void** d_count,
                                          const void** d_verdict, uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_clean_device_impl(c, min_count, max_count, max_tip_keys, max_island_keys, d_key_hi, d_key_lo, d_count, d_verdict, n_kept,
                                            n_unitigs, summary, {max_bubble_keys, KMC_SIMPLIFY_WORDS, true, "kmc_unitig_simplify_device"});
    });
}
extern "C" int kmc_unitig_simplify(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                                   uint64_t max_bubble_keys, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap_keys,
                                   uint8_t* verdict, uint64_t cap_unitigs, uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_clean_impl(c, min_count, max_count, max_tip_keys, max_island_keys, key_hi, key_lo, count, cap_keys, verdict, cap_unitigs,
                                     n_kept, n_unitigs, summary, {max_bubble_keys, KMC_SIMPLIFY_WORDS, true, "kmc_unitig_simplify"});
    });
}
extern "C" int kmc_unitig_simplify_into(kmc_ctx* src, kmc_ctx* dst, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys,
                                        uint64_t max_island_keys, uint64_t max_bubble_keys, uint64_t* summary) {
    return guarded(src, [&]() -> int {
        return kmc_unitig_clean_into_impl(src, dst, min_count, max_count, max_tip_keys, max_island_keys, summary,
                                          {max_bubble_keys, KMC_SIMPLIFY_WORDS, true, "kmc_unitig_simplify_into"});
    });
}
extern "C" int kmc_unitig_components_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_component_keys,
                                            const void** d_comp_of, const void** d_comp_stats, const void** d_verdict, const void** d_key_hi,
                                            const void** d_key_lo, const void** d_count, uint64_t* n_comps, uint64_t* n_unitigs, uint64_t* n_kept,
                                            uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_components_device_impl(c, min_count, max_count, max_component_keys, d_comp_of, d_comp_stats, d_verdict, d_key_hi, d_key_lo,
                                                 d_count, n_comps, n_unitigs, n_kept, summary);
    });
}
extern "C" int kmc_unitig_components(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_component_keys, uint32_t* comp_of,
                                     uint8_t* verdict, uint64_t cap_unitigs, uint64_t* comp_stats, uint64_t cap_comps, uint64_t* key_hi,
                                     uint64_t* key_lo, uint64_t* count, uint64_t cap_keys, uint64_t* n_comps, uint64_t* n_unitigs, uint64_t* n_kept,
                                     uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_components_impl(c, min_count, max_count, max_component_keys, comp_of, verdict, cap_unitigs, comp_stats, cap_comps, key_hi,
                                          key_lo, count, cap_keys, n_comps, n_unitigs, n_kept, summary);
    });
}
extern "C" int kmc_unitig_components_into(kmc_ctx* src, kmc_ctx* dst, uint64_t min_count, uint64_t max_count, uint64_t max_component_keys,
                                          uint64_t* summary) {
    return guarded(src, [&]() -> int { return kmc_unitig_components_into_impl(src, dst, min_count, max_count, max_component_keys, summary); });
}
extern "C" int kmc_unitig_bubbles_device(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_bubble_keys, const void** d_records,
                                         uint64_t* n_records, uint64_t* n_unitigs, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_bubbles_device_impl(c, min_count, max_count, max_bubble_keys, d_records, n_records, n_unitigs, summary);
    });
}
extern "C" int kmc_unitig_bubbles(kmc_ctx* c, uint64_t min_count, uint64_t max_count, uint64_t max_bubble_keys, uint32_t* records,
                                  uint64_t cap_records, uint64_t* n_records, uint64_t* n_unitigs, uint64_t* summary) {
    return guarded(c, [&]() -> int {
        return kmc_unitig_bubbles_impl(c, min_count, max_count, max_bubble_keys, records, cap_records, n_records, n_unitigs, summary);
    });
}
extern "C" int kmc_partition_device(kmc_ctx* c, uint32_t n_parts, uint64_t* part_begin, const void** d_key_hi,
                                    const void** d_key_lo, const void** d_count) {
    return guarded(c, [&]() -> int { return kmc_partition_device_impl(c, n_parts, part_begin, d_key_hi, d_key_lo, d_count); });
}
