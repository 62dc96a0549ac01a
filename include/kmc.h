/*
 * kmc.h -- C ABI of the MI355X k-mer counter (libkmc.so).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (jaxonwang/k-mer-count @ v1, paths below relative to /root/reference) has no FFI of its own:
 * its whole pipeline is one function, k-mer-count/src/main.rs:43-91.  The entry points below
 * are what a Rust `extern "C"` block in that crate would bind so that main() keeps FASTA
 * reading (main.rs:44-46,58-62) and printing (main.rs:88-90) and hands the loop nest in
 * between (main.rs:63-87) to the GPU.  INTEGRATION.md shows the binding.
 *
 *   reference code being replaced                         entry point
 *   ----------------------------------------------------  ---------------------------------
 *   constants l_len/r_len/80..141, main.rs:48-49,63       kmc_create(kmc_config)
 *   per-record window loop + push, main.rs:58-81          kmc_add_batch / kmc_add_batch_device
 *   radix_sort + sort (grouping), main.rs:84,87           kmc_finalize
 *   iteration over the sorted result, main.rs:88-90       kmc_export (sorted ascending)
 *   File::open + Reader + loop, main.rs:44-46,58-62       kmc_count_file (convenience; host parser)
 *   random_fasta_generator.py:5-15                        kmc_synth_* (seeded, sized re-creation)
 *   (addition: no equivalent in the reference)             kmc_histogram (abundance histogram of the view)
 *   (addition: no equivalent in the reference)             kmc_filter_device / kmc_export_filtered (count range)
 *   (addition: no equivalent in the reference)             kmc_encode_key (ASCII k-mer -> packed key)
 *   (addition: no equivalent in the reference)             kmc_query / kmc_query_device (count of given keys)
 *   (addition: no equivalent in the reference)             kmc_profile / kmc_profile_device (per-read k-mer profile)
 *   (addition: no equivalent in the reference)             kmc_compare / kmc_setop_device / kmc_export_setop (two tables)
 *   (addition: no equivalent in the reference)             kmc_graph / kmc_graph_device (de Bruijn graph of the table)
 *   (addition: no equivalent in the reference)             kmc_unitigs / kmc_unitigs_device (its unitig sequences)
 *   (addition: no equivalent in the reference)             kmc_unitig_links / kmc_unitig_links_device (the edges between them)
 *   (addition: no equivalent in the reference)             kmc_unitig_clean / kmc_unitig_clean_device / kmc_unitig_clean_into (tips and islands removed)
 *   (addition: no equivalent in the reference)             kmc_unitig_simplify / kmc_unitig_simplify_device / kmc_unitig_simplify_into (and simple bubbles popped)
 *   (addition: no equivalent in the reference)             kmc_unitig_components (connected components of the unitig graph, the small ones dropped)
 *   (addition: no equivalent in the reference)             kmc_unitig_components_device (the same in ctx-owned device memory)
 *   (addition: no equivalent in the reference)             kmc_unitig_components_into (the table without small components, into another ctx)
 *   (addition: no equivalent in the reference)             kmc_unitig_bubbles / kmc_unitig_bubbles_device (its bubbles reported as variant records)
 *   (addition: no equivalent in the reference)             kmc_unitig_map / kmc_unitig_map_device (reads threaded through the unitigs)
 *   (addition: no equivalent in the reference)             kmc_unitig_transits / kmc_unitig_transits_device (read walks counted per link and per unitig)
 *   (addition: no equivalent in the reference)             kmc_unitig_contigs / kmc_unitig_contigs_device (resolved repeats duplicated, unsupported links cut, contigs spelled)
 *   (addition: no equivalent in the reference)             kmc_unitig_pairs / kmc_unitig_pairs_device (pair evidence: the ends mates connect, the bases between them, insert sizes)
 *   (addition: no equivalent in the reference)             kmc_correct / kmc_correct_device (substitution errors of reads repaired from the table)
 *   (addition: no equivalent in the reference)             kmc_trim / kmc_trim_device (reads trimmed and filtered by their solid k-mers)
 *   (addition: no equivalent in the reference)             kmc_normalize / kmc_normalize_device (read depth normalised: a per-read k-mer depth, deep reads sampled down)
 *
 * Conventions
 *   - Every function returns 0 (KMC_OK) or a negative kmc_status; no exception or abort crosses
 *     the ABI (the reference panics instead: main.rs:23,35,44,59).
 *   - Alphabet A=0 C=1 G=2 T=3 (main.rs:19-22); keys are packed MSB-first so unsigned order of
 *     (key_hi,key_lo) equals the reference's string order (main.rs:87).  key_hi is 0 for k<=32.
 *   - The caller owns every host buffer passed in or out; buffers passed to kmc_add_batch may be
 *     reused as soon as it returns.  The library owns the ctx and all device memory.
 *   - A ctx is bound to ONE GPU and is not thread-safe; distinct ctxs are independent.
 *   - There is NO CPU fallback: if no HIP device is usable kmc_create fails with
 *     KMC_ERR_NO_DEVICE.
 */
#ifndef KMC_H
#define KMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMC_VERSION_MAJOR 0
#define KMC_VERSION_MINOR 1

typedef enum kmc_status {
    KMC_OK = 0,
    KMC_ERR_ARG = -1,        /* bad argument / unsupported k */
    KMC_ERR_NO_DEVICE = -2,  /* no usable HIP device (no CPU fallback exists) */
    KMC_ERR_HIP = -3,        /* a HIP runtime call failed; see kmc_last_error */
    KMC_ERR_NOMEM = -4,      /* host or device allocation failed */
    KMC_ERR_IO = -5,         /* cannot open/read file            (main.rs:44) */
    KMC_ERR_FORMAT = -6,     /* "Expected > at record start."    (main.rs:59) */
    KMC_ERR_ALPHABET = -7,   /* non-ACGT byte in LR mode         (main.rs:23) */
    KMC_ERR_CAPACITY = -8,   /* count table and spill area exhausted; a view of 2^32 keys or more
                                (the sort's own lists are sized from a bound: no input overflows them) */
    KMC_ERR_STATE = -9       /* call out of order (e.g. export before finalize) */
} kmc_status;

typedef enum kmc_mode {
    KMC_MODE_CONTIG = 0, /* contiguous k-mers, SURVEY.md 8a-def */
    KMC_MODE_LR = 1      /* reference mode: 27 + gap + 27, chunk sizes 80..=140 (main.rs:48-49,63) */
} kmc_mode;

typedef enum kmc_algo {
    KMC_ALGO_AUTO = 0,   /* pick per batch: WALK for short reads, SORT once the input proves high-cardinality, else STREAM */
    KMC_ALGO_STREAM = 1, /* per-k-mer LDS partial histogram + global atomics (any input) */
    KMC_ALGO_WALK = 2,   /* memoised successor walk: one LDS lookup per 16 bases (longer reads as overlapping pieces of 416) */
    KMC_ALGO_SORT = 3    /* extract every window; batches accumulate; hand-written MSD radix sort + run-length when the
                            result is needed (high-cardinality input) */
} kmc_algo;

/* Deviations from the config sketched in SURVEY.md 8b (`n_devices`, `device_ids*`, `backend`), on purpose:
 *   - ONE `device` per ctx instead of n_devices/device_ids: a ctx is one GPU's table and stream.  Several
 *     GPUs of one process = several ctxs handed to kmc_count_file_multi (the CLI's --gpus N); scaling
 *     runs use one process per GPU and RCCL (kmc_pack_slab_device / kmc_merge_slabs_device /
 *     kmc_partition_device are the device-side halves of that reduce).
 *   - no `backend` field and no `--backend cpu`: the library has no CPU path to select (kmc_create
 *     fails with KMC_ERR_NO_DEVICE instead); the CPU restatement lives in oracle/ as test infrastructure.
 *   - `algo` and `stream` are additions (kernel choice for measurements; running on the caller's stream so
 *     that kernels and collectives are ordered on the device).
 * Alphabet rule of KMC_MODE_LR: the reference panics on a character outside ACGT that its bucket_sort
 * inspects (main.rs:17-23: chunk indices 1..53 of every emitted chunk).  Here KMC_ERR_ALPHABET is raised
 * for such a byte at ANY index of an emitted chunk (index 0 too: a 2-bit key cannot hold it); bytes no
 * window reads -- reads shorter than 80 bases, the uncovered middle of reads of 80..105 bases -- are
 * accepted, as in the reference.  KMC_MODE_CONTIG skips windows that contain such a byte (8a-def). */
typedef struct kmc_config {
    uint32_t struct_size;   /* = sizeof(kmc_config) */
    int32_t  k;             /* 1..63 in KMC_MODE_CONTIG; ignored in KMC_MODE_LR */
    int32_t  mode;          /* kmc_mode */
    int32_t  canonical;     /* 1: key = min(fwd, revcomp); 0: forward strand (the reference is forward-only) */
    int32_t  device;        /* HIP device ordinal */
    int32_t  algo;          /* kmc_algo */
    uint64_t capacity_hint; /* expected distinct keys; 0 = default.  The table grows between batches. */
    void*    stream;        /* hipStream_t to run on, or NULL for a ctx-owned stream */
} kmc_config;

typedef struct kmc_ctx kmc_ctx;

/* Per-ctx counters, all cumulative since kmc_create / kmc_reset. */
typedef struct kmc_stats {
    uint64_t n_reads;
    uint64_t n_bases;
    uint64_t n_kmers;         /* valid windows counted (== sum of counts) */
    uint64_t n_distinct;      /* valid after kmc_finalize */
    uint64_t table_capacity;  /* slots */
    uint64_t n_spilled;       /* pairs that went through the spill area */
    uint64_t n_batches;
    double   kernel_ms_last;  /* sum of hipEvent-bracketed count-kernel launches of the last batch */
    double   kernel_ms_total;
    int32_t  algo_last;       /* kmc_algo actually used for the last batch */
    int32_t  launches_last;   /* count-kernel launches in the last batch */
    uint64_t n_slabs_skipped; /* oversize slabs seen by kmc_merge_slabs_device (valid after kmc_finalize) */
    uint64_t n_direct;        /* k-mers the WALK / STREAM kernels counted with one global atomic each because their
                                 LDS memo / partial table was full (valid after kmc_finalize / kmc_poll) */
    double   kernel_ms_lifetime;  /* like kernel_ms_total, but since kmc_create: kmc_reset does not clear it (a caller that */
    uint64_t launches_lifetime;   /* resets the ctx per step reads the kernel time of all steps once, after the last) */
    uint64_t n_async_ok;          /* finalizes of this ctx that produced their view through the small-table kernel, and the oversize */
    uint64_t n_async_slabs_skipped; /* slabs they saw, both since kmc_create (as of the last call that synchronised): see kmc_finalize_async */
    uint64_t n_planner_stale;     /* debug invariant of the launch planner: risky launches whose table snapshot was armed on
                                     counters older than the last queued unfold / merge (must stay 0) */
    uint64_t walk_uniform_launches; /* walk-kernel launches since kmc_create (kmc_reset does not clear it) that ran the
                                       uniform-length variant: all reads of the batch equally long, no offsets read */
    uint64_t walk_plan_finalizes;   /* finalizes since kmc_create (kmc_reset does not clear them) whose view the walk path's plan
                                       launch wrote: a repeat batch gathered from its rank plan, no table, no sort */
    uint64_t walk_plan_builds;      /* rank plans built (queued) since kmc_create */
} kmc_stats;

const char* kmc_version(void);
const char* kmc_status_string(int status);

int  kmc_create(kmc_ctx** out, const kmc_config* cfg);
void kmc_destroy(kmc_ctx* ctx);
/* Message of the last failing call on this ctx (owned by the ctx; "" if none).  ctx may be NULL:
 * then the message of the last failing kmc_create on this thread. */
const char* kmc_last_error(const kmc_ctx* ctx);

/* Forget all counts (table kept allocated). */
int kmc_reset(kmc_ctx* ctx);

/* Count one batch of reads.  `bases`: ASCII bases of all reads concatenated (no newlines);
 * `offsets[n_reads+1]`: start of each read, offsets[0] == 0, offsets[n_reads] == total bases.
 * Host buffers; copied to the device before return. */
int kmc_add_batch(kmc_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads);

/* Same, for buffers already resident in this ctx's GPU memory (HBM-resident timing, pipelines
 * that parse into pinned/device memory).  d_bases must be 16-byte aligned and readable up to the
 * next 16-byte boundary past the last base.  max_read_len: longest read in the batch, or 0 if
 * unknown (then it is computed on the device).  A non-zero max_read_len MUST be >= the length of every read
 * of the batch, and the library relies on it: the launch planner's bounds and the walk kernel's 416-base staging
 * area are sized by it, and a batch with n_bases == n_reads * max_read_len is taken to consist of reads of exactly
 * that length each, whose bounds the walk kernel then computes instead of loading d_offsets (d_offsets must be
 * valid all the same: other parts of the path read it).  Asynchronous on the ctx stream.  The buffers must stay
 * valid and unchanged until the next call on this ctx that synchronises (kmc_add_batch*, kmc_finalize,
 * kmc_poll, kmc_export): the batch may go out in one launch sized by what earlier batches looked like, and
 * if that prediction proves wrong (far more distinct k-mers than the table and its spill area hold) the
 * library puts the table back and counts the affected part of the batch again by sorting -- nothing is
 * dropped and no KMC_ERR_CAPACITY is raised. */
int kmc_add_batch_device(kmc_ctx* ctx, const void* d_bases, const void* d_offsets,
                         uint64_t n_reads, uint64_t n_bases, uint64_t max_read_len);

/* Merge (key,count) pairs that already live on this GPU into the table (multi-GPU reduce:
 * pairs received from a peer over RCCL).  d_key_hi may be NULL when k <= 32 / not LR. */
int kmc_merge_pairs_device(kmc_ctx* ctx, const void* d_key_hi, const void* d_key_lo,
                           const void* d_count, uint64_t n_pairs);

/* Compact the table, sort by key on the device, report sizes.  May be called repeatedly;
 * more batches may be added afterwards (the sorted view is then stale until the next finalize).
 * A call that finds nothing added, merged or reset since the last finalize makes NO new view when that finalize went the
 * small-table way (it emptied the table into the view: tables up to some ten thousand keys, the empty one included, and
 * every view kmc_finalize_async queued): it reports the sizes of the view in place and changes nothing.  Where this header
 * says that "finalize" ends the validity of a device pointer, drops a result a ctx holds or makes a call compute again,
 * such a call is not meant: the pointers stay valid, a host form still copies what is held and KMC_TRANSIT_ACCUMULATE or
 * KMC_PAIR_ACCUMULATE still finds its result.  A larger table is compacted and sorted again: a new view, with everything that says. */
int kmc_finalize(kmc_ctx* ctx, uint64_t* n_distinct, uint64_t* n_total);

/* kmc_finalize for a pipeline that does not want to wait: the device work of a SMALL table's finalize (at most 131072
 * keys, nothing spilled: every table of generator-style input) is queued on the ctx stream and the call returns.  Behind
 * it in stream order the sorted view is in place (the pointers kmc_export_device last returned stay valid for small
 * tables) and the table is empty; kmc_reset after it launches one small kernel and does not wait either.  The next call
 * that needs the outcome on the host (kmc_finalize, kmc_export*, kmc_add_batch*, kmc_merge_pairs_device, kmc_count_file,
 * kmc_poll, the spectrum calls, ...) synchronises once and takes it from there -- kmc_finalize then returns the sizes of
 * the view this call produced; a call that reads the view gets it also when the device found the table too large, by
 * the ordinary finalize; an addition puts the view's counts back into the table first.  A caller that queues many steps
 * (count -> kmc_finalize_async -> kmc_reset -> ...) checks afterwards that every step delivered:
 * kmc_stats.n_async_ok grows by one per finalize that produced its view, n_async_slabs_skipped by the oversize slabs
 * those finalizes saw (both valid after a synchronising call).  An empty table (nothing spilled, nothing pending) produces
 * its view too, the empty one: a reduce step whose owner holds no key counts as delivered, and the oversize slabs it saw
 * are counted.  Larger tables are finalized synchronously, as by kmc_finalize. */
int kmc_finalize_async(kmc_ctx* ctx);

/* Copy the sorted table to caller-allocated host arrays of `cap` entries (cap >= n_distinct).
 * key_hi may be NULL if the caller knows k <= 32. */
int kmc_export(kmc_ctx* ctx, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap);

/* Device pointers to the sorted table of the last kmc_finalize (owned by the ctx, valid until the
 * next finalize/reset/destroy).  d_key_hi is NULL when keys fit one word.
 * Ordering contract: when kmc_export_device returns, every kernel that writes the view has FINISHED, so the arrays may
 * be read from any stream, by a peer copy or by a collective without further synchronisation.  (kmc_finalize itself may
 * return earlier than that for a small table: its kernel tells the host through pinned memory that the view and the
 * counters are complete while it is still clearing table slots -- work queued on the ctx stream is ordered behind it
 * anyway, and this call waits for the kernel's end, once, before it hands out pointers.) */
int kmc_export_device(kmc_ctx* ctx, const void** d_key_hi, const void** d_key_lo,
                      const void** d_count, uint64_t* n_distinct);

/* Owner-partitioned view for an all-to-all exchange: after kmc_finalize, reorders the sorted
 * table so that pairs with owner(key) == p are contiguous, p = 0..n_parts-1, where
 * owner = mix(key) % n_parts (kmc_owner_of gives the same function on the host).
 * part_begin[n_parts+1] (host) receives the boundaries.  Pointers as in kmc_export_device. */
int kmc_partition_device(kmc_ctx* ctx, uint32_t n_parts, uint64_t* part_begin,
                         const void** d_key_hi, const void** d_key_lo, const void** d_count);
uint32_t kmc_owner_of(uint64_t key_hi, uint64_t key_lo, uint32_t n_parts);

/* ---- what comes after counting (additions: the reference prints its whole table, main.rs:88-90) ----
 * All three read the sorted view of the last kmc_finalize (a view queued by kmc_finalize_async counts as one) and
 * change neither it nor a kmc_partition_device result.  A NULL ctx is KMC_ERR_ARG, no view KMC_ERR_STATE, a non-zero
 * max_count below min_count KMC_ERR_ARG; an empty view gives zeros. */

/* Abundance histogram of the sorted view (after kmc_finalize): for 0 <= c < n_bins-1, hist[c] = number of keys with
 * count == c; hist[n_bins-1] = number with count >= n_bins-1 (hist[0] is always 0).  Only keys with
 * min_count <= count <= max_count are counted (max_count 0 = no upper bound).  *max_seen (may be NULL) = largest
 * count in range, 0 if none.  2 <= n_bins <= 2^24. */
int kmc_histogram(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint32_t n_bins, uint64_t* hist, uint64_t* max_seen);

/* Keys of the sorted view with min_count <= count <= max_count (max_count 0 = no upper bound), in view order, in
 * ctx-owned device arrays valid until the next kmc_filter_device / kmc_export_filtered / finalize / reset / destroy
 * (same ordering contract as kmc_export_device; d_key_hi is NULL when keys fit one word).  A filter that keeps
 * everything (min_count <= 1, max_count 0) launches nothing and returns the kmc_export_device pointers.
 * *n_kept / *kept_total (may be NULL) = entries kept and the sum of their counts. */
int kmc_filter_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, const void** d_key_hi,
                      const void** d_key_lo, const void** d_count, uint64_t* n_kept, uint64_t* kept_total);

/* The same, copied to caller arrays of `cap` entries (key_hi may be NULL if the caller knows k <= 32).  *n_kept is
 * always set; cap < *n_kept -> KMC_ERR_ARG and nothing is copied (call with cap 0 and NULL arrays to size the buffers). */
int kmc_export_filtered(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t* key_hi, uint64_t* key_lo,
                        uint64_t* count, uint64_t cap, uint64_t* n_kept);

/* ---- asking the table: key lookups and per-read profiles (additions, as above: they read the sorted view of the last
 * kmc_finalize -- a view queued by kmc_finalize_async counts as one -- and change neither the table, the view, a
 * kmc_partition_device result nor a kmc_filter_device result).  A NULL ctx is KMC_ERR_ARG, no view KMC_ERR_STATE (exactly
 * where kmc_export says so), an empty view gives zeros.  The first query of a view builds a prefix index over it on the
 * device (kept by the ctx until its next view); a view of 2^32 keys or more is KMC_ERR_CAPACITY. ---- */

/* ASCII k-mer -> packed key (inverse of kmc_decode_key).  canonical != 0: min(fwd, revcomp).  Host only, no ctx.
 * klen outside 1..63 or a null pointer: KMC_ERR_ARG; a byte outside upper-case ACGT: KMC_ERR_ALPHABET. */
int kmc_encode_key(const char* kmer, int klen, int canonical, uint64_t* key_hi, uint64_t* key_lo);

/* count[i] = count of key i in the sorted view of the last finalize, 0 if absent.  Keys are looked up AS GIVEN
 * (in a canonical ctx a non-canonical key is simply absent).  key_hi may be NULL when keys fit one word.
 * Any order, duplicates allowed, n_keys == 0 is fine. */
int kmc_query(kmc_ctx* ctx, const uint64_t* key_hi, const uint64_t* key_lo, uint64_t n_keys, uint64_t* count);
/* Same on device arrays of this ctx's GPU (8-byte aligned; 16-byte aligned arrays are read and written 16 bytes per lane);
 * asynchronous on the ctx stream, no host synchronisation of its own beyond what resolving the view needs. */
int kmc_query_device(kmc_ctx* ctx, const void* d_key_hi, const void* d_key_lo, uint64_t n_keys, void* d_count);

#define KMC_PROFILE_WORDS 5
/* Per-read k-mer profile of a batch (same bases/offsets layout as kmc_add_batch) against the view; the batch is NOT
 * counted.  KMC_MODE_CONTIG only (LR: KMC_ERR_ARG).  Uses the ctx's k and canonical setting.
 *   window_count[n_bases] (may be NULL): entry offsets[r] + j = count of the window that STARTS at base j of read r,
 *     saturated at 0xFFFFFFFF; 0 for an absent key, for a window containing a byte outside ACGT, and for the last
 *     k-1 positions of a read (all positions of a read shorter than k).
 *   read_stats[n_reads * KMC_PROFILE_WORDS] (may be NULL), per read: [0] valid windows (no non-ACGT byte),
 *     [1] of those, windows with count >= max(min_count, 1), [2] smallest and [3] largest count over the valid
 *     windows (absent = 0; both 0 when there is no valid window), [4] sum of counts.  [2..4] are exact u64. */
int kmc_profile(kmc_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t min_count,
                uint32_t* window_count, uint64_t* read_stats);
/* Device form: alignment / padding rules of kmc_add_batch_device for d_bases; asynchronous on the ctx stream. */
int kmc_profile_device(kmc_ctx* ctx, const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
                       uint64_t min_count, void* d_window_count, void* d_read_stats);

/* ---- two tables: summary and set operations (additions, as above).  A and B are the sorted views of the last
 * kmc_finalize of two contexts (a view queued by kmc_finalize_async counts as one).  For a key x, ca = its count in A if
 * it is present there and min_a <= count <= max_a (max_a 0 = no upper bound), else 0; cb likewise with min_b / max_b.
 * Only keys with ca != 0 or cb != 0 exist for the operation.
 *   op          KMC_SETOP_INTERSECT: ca != 0 && cb != 0;  KMC_SETOP_UNION: ca != 0 || cb != 0;  KMC_SETOP_SUBTRACT: ca != 0 && cb == 0
 *   count_mode  result count r = ca (LEFT), cb (RIGHT), min(ca, cb), max(ca, cb), ca + cb (SUM: plain 64-bit addition),
 *               ca > cb ? ca - cb : 0 (DIFF)
 * A selected key is emitted iff r != 0, in ascending key order: the result has the shape of a view (UNION + DIFF is
 * "counter subtract"; UNION + LEFT with ranges is A filtered).
 * Rules: a NULL context, an unknown op / count_mode, a non-zero max below its min: KMC_ERR_ARG.  a and b must agree in
 * device, mode, k and canonical (KMC_ERR_ARG; the message names the field); a == b is allowed.  No view: KMC_ERR_STATE
 * (message on the ctx that lacks it).  The two views together must hold fewer than 2^32 keys (KMC_ERR_CAPACITY).  Work
 * runs on a's stream and the result lives in device arrays owned by a, valid until the next set operation / finalize /
 * reset / destroy of a (same ordering contract as kmc_export_device; d_key_hi is NULL when keys fit one word).  b's view
 * is only read.  Neither view, nor a partition, filter result or query index of either context is changed. ---- */
#define KMC_SETOP_INTERSECT 0
#define KMC_SETOP_UNION 1
#define KMC_SETOP_SUBTRACT 2
#define KMC_COUNT_LEFT 0
#define KMC_COUNT_RIGHT 1
#define KMC_COUNT_MIN 2
#define KMC_COUNT_MAX 3
#define KMC_COUNT_SUM 4
#define KMC_COUNT_DIFF 5
#define KMC_COMPARE_WORDS 8
/* summary[KMC_COMPARE_WORDS]: [0] n_a = keys with ca != 0, [1] n_b, [2] n_both, [3] sum of ca, [4] sum of cb, [5] sum of ca
 * over shared keys, [6] sum of cb over shared keys, [7] sum of min(ca, cb).  It does not depend on op / count_mode.
 * Union size n_a + n_b - n_both, Jaccard n_both / union, containment n_both / n_a, weighted Jaccard
 * [7] / ([3] + [4] - [7]) and the Bray-Curtis similarity 2 [7] / ([3] + [4]) are host arithmetic on it. */
int kmc_compare(kmc_ctx* a, kmc_ctx* b, uint64_t min_a, uint64_t max_a, uint64_t min_b, uint64_t max_b, uint64_t* summary);
/* *n_out / *total_out (may be NULL) = entries of the result and the sum of their counts; summary may be NULL. */
int kmc_setop_device(kmc_ctx* a, kmc_ctx* b, int op, int count_mode, uint64_t min_a, uint64_t max_a, uint64_t min_b,
                     uint64_t max_b, const void** d_key_hi, const void** d_key_lo, const void** d_count, uint64_t* n_out,
                     uint64_t* total_out, uint64_t* summary);
/* The same, copied to caller arrays of `cap` entries (key_hi may be NULL if the caller knows k <= 32).  *n_out is always
 * set; cap < *n_out -> KMC_ERR_ARG and nothing is copied (call with cap 0 and NULL arrays to size the buffers). */
int kmc_export_setop(kmc_ctx* a, kmc_ctx* b, int op, int count_mode, uint64_t min_a, uint64_t max_a, uint64_t min_b,
                     uint64_t max_b, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap, uint64_t* n_out);

/* ---- the table as a de Bruijn graph: neighbour masks and unitig ends (additions, as above).  KMC_MODE_CONTIG only (LR:
 * KMC_ERR_ARG), every k, canonical or forward ctx.  Write a key as its k-character string x.  canon(f) = min(f, revcomp(f))
 * as strings in a canonical ctx, f itself in a forward ctx (the ctx's own key rule, kmc_encode_key).  A key is SOLID iff it
 * is in the sorted view of the last kmc_finalize (a view queued by kmc_finalize_async counts as one) and
 * min_count <= count <= max_count (max_count 0 = no upper bound), the range rule of kmc_filter_device.
 * For a solid key x, side R (right) and side L (left), base c in ACGT (codes 0..3):
 *   ext(x, R, c) = canon(x[1:] + c),  ext(x, L, c) = canon(c + x[:-1]).
 *   bit c of adj (bits 0..3) is set iff ext(x, R, c) is solid; bit 4 + c (bits 4..7) iff ext(x, L, c) is solid.  Degrees are
 *     the popcounts of the two nibbles: they count BASES, not distinct neighbour keys.  Self-loops (homopolymers) and
 *     palindromes get no special case: the formula is the definition.
 *   facing side: if f = x[1:] + c (or c + x[:-1]) was kept as it is by canon, the neighbour y is entered on the opposite
 *     side (an R-extension enters y on its L side and vice versa); if canon flipped it, on the same side.
 *   side S of x CONTINUES iff its degree is 1 and the facing side of that one neighbour has degree 1 too.  Otherwise side
 *     S is a UNITIG END: bit 8 (R) / bit 9 (L).
 *   bit 10 = the key is solid.  A key of the view that is not solid gets adj = 0.  Bits 11..15 are 0.
 * adj is one uint16_t per key OF THE VIEW, IN VIEW ORDER (entry i belongs to row i of kmc_export).
 * summary[KMC_GRAPH_WORDS], over solid keys: [0] nodes, [1] sum of R degrees, [2] sum of L degrees, [3] isolated nodes (both
 * degrees 0), [4] dead ends (exactly one degree 0), [5] branching nodes (a degree >= 2), [6] unitig-end sides (bits 8 and 9
 * summed), [7] nodes with both end bits set (single-node unitigs).  Non-circular unitigs = [6] / 2 is host arithmetic.
 * Rules: a NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no view: KMC_ERR_STATE (exactly where
 * kmc_export says so); a view of 2^32 keys or more: KMC_ERR_CAPACITY (the prefix index's rule; the first graph or query call
 * of a view builds the index, the other reuses it); an empty view gives zeros.  The table, the view, a partition, a filter
 * result, a set-operation result and the query index are not changed. ---- */
#define KMC_GRAPH_WORDS 8
#define KMC_GRAPH_RIGHT(adj) ((adj) & 15u)
#define KMC_GRAPH_LEFT(adj) (((adj) >> 4) & 15u)
#define KMC_GRAPH_END_R(adj) (((adj) >> 8) & 1u)
#define KMC_GRAPH_END_L(adj) (((adj) >> 9) & 1u)
#define KMC_GRAPH_SOLID(adj) (((adj) >> 10) & 1u)
/* adj in a ctx-owned device array of uint16_t, valid until the next kmc_graph* or kmc_unitigs* call / finalize / reset / destroy (same
 * ordering contract as kmc_export_device).  d_adj, n_keys (keys of the view) and summary may each be NULL. */
int kmc_graph_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, const void** d_adj, uint64_t* n_keys,
                     uint64_t* summary);
/* The same, copied to the caller's array adj of cap uint16_t entries.  *n_keys is always set; cap < *n_keys -> KMC_ERR_ARG and
 * nothing is copied, except that adj == NULL with cap == 0 is the summary-only / sizing call.  summary may be NULL. */
int kmc_graph(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, void* adj, uint64_t cap, uint64_t* n_keys,
              uint64_t* summary);

/* ---- the unitigs of that graph: the maximal non-branching paths spelled out (additions, as above).  KMC_MODE_CONTIG only,
 * every k, canonical or forward ctx; the solidity range and the adj words are those of kmc_graph.
 * SIDE STATES.  a = 2 * row + s, row the view row of a solid key, s = 0 for side R, 1 for side L; a ^ 1 is the other side of
 *   the same key.
 * PARTNER AND JOIN.  partner(a) is defined iff side a continues (its end bit in adj is clear): it is (y, T), the one solid
 *   neighbour y on that side and the side T of y that faces back (the facing-side rule above).  Side a is JOINED to
 *   b = partner(a) iff partner(b) is defined, partner(b) == a and b != a; otherwise a is a TERMINAL.  The mutual check
 *   matters: in a canonical ctx a k-mer whose extension is its own reverse complement is its own partner on the same side
 *   (a hairpin), and for even k a palindromic k-mer makes two of its sides claim the same partner.
 * SHAPE.  Joins are a symmetric matching on sides; with each key's own pair of sides the solid keys fall into disjoint
 *   simple paths and simple cycles.
 * CIRCULAR UNITIGS.  A cycle is cut on the L side of its smallest-row key m: side (m, L) and the side it was joined to
 *   become terminals, the unitig is marked circular, and from there on it is a path.
 * ORIENTATION AND SPELLING.  A path with end keys of rows r1, r2 (equal for a one-key unitig) starts at the end key of the
 *   smaller row and moves away from that key's terminal side; in a forward ctx, or when r1 == r2, the direction that leaves
 *   keys through side R is used (in a forward ctx the only one that spells a string).  The first key contributes its k
 *   characters -- as stored if it is left through R, its reverse complement if left through L -- and every further key one
 *   character, the last of its reading in that same sense.  A unitig of m keys has m + k - 1 bases; a circular one is
 *   spelled linearly from the cut.
 * ORDER.  Unitigs are numbered by the view row of their first key, ascending.  Every solid key occurs in exactly one
 *   unitig, exactly once.
 * Outputs: bases (ASCII ACGT, concatenated) with offsets[n_unitigs + 1], offsets[0] == 0 -- the layout kmc_add_batch takes;
 * abund[u] = the sum of the counts of unitig u's keys (exact; the mean is host arithmetic); flags[u] bit 0
 * (KMC_UNITIG_CIRCULAR) = circular.  summary[KMC_UNITIG_WORDS]: [0] unitigs, [1] bases, [2] keys (= solid keys), [3] circular
 * unitigs, [4] one-key unitigs, [5] keys of the longest unitig, [6] sides that continue in adj but are not joined (hairpins,
 * palindromes), [7] sum of abund.  With g the kmc_graph summary of the same range: [1] == [2] + (k - 1) * [0] and
 * 2 * [0] == g[6] + [6] + 2 * [3].
 * Rules: those of kmc_graph (NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no view:
 * KMC_ERR_STATE exactly where kmc_export says so; an empty view gives zeros), except that a view of 2^31 keys or more is
 * KMC_ERR_CAPACITY (a side state is a u32).  The table, the view, a partition, a filter result, a set-operation result and
 * the query index are not changed.  The adj array of kmc_graph_device IS rewritten: kmc_unitigs* counts as a kmc_graph*
 * call (it leaves the adj words of its own range there whenever it computes: see kmc_unitigs for the one time it does not).
 * Diagnostic: with KMC_UNITIG_TRACE set in the environment, every call that computes also prints one line to stderr,
 * "kmc_unitigs: keys N rounds R cycle_states S adj_ms .. links_ms .. ranking_ms .. cycles_ms .. layout_ms .. emit_ms ..":
 * its own phase times from event pairs on the ctx's stream, read at the end of the call (tools/measure_unitigs.py reads
 * them).  It changes no result, queue or graph; unset, it costs one getenv per call. ---- */
#define KMC_UNITIG_WORDS 8
#define KMC_UNITIG_CIRCULAR 1u      /* bit 0 of a flags byte */
/* The four arrays in ctx-owned device memory -- uint8_t bases[n_bases], uint64_t offsets[n_unitigs + 1], uint64_t
 * abund[n_unitigs], uint8_t flags[n_unitigs] -- valid until the next kmc_unitigs* call / finalize / reset / destroy (same
 * ordering contract as kmc_export_device).  d_bases / d_offsets obey the alignment and padding rule of kmc_add_batch_device:
 * they can be handed to kmc_add_batch_device / kmc_profile_device of another ctx on this device.  Every output pointer may
 * be NULL. */
int kmc_unitigs_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, const void** d_bases, const void** d_offsets,
                       const void** d_abund, const void** d_flags, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* summary);
/* The same, copied to the caller's arrays: bases of cap_bases bytes; offsets of cap_unitigs + 1, abund and flags of cap_unitigs
 * entries.  Every output pointer may be NULL (an array that is NULL is not copied and its cap not looked at).  *n_unitigs and
 * *n_bases are always set; a cap too small for an array that was given -> KMC_ERR_ARG and nothing is copied.  All arrays NULL
 * (caps 0) is the sizing / summary-only call.
 * Cost: a call computes everything on the device, whatever it copies -- except that a kmc_unitigs call whose ctx still holds
 * the result of the last kmc_unitigs* call for this very view and range copies from that result instead.  So the sizing
 * call followed by the call that copies computes once, not twice; any finalize, or a kmc_unitigs* call with another
 * range, in between makes the second call compute again.  kmc_unitigs_device always computes. */
int kmc_unitigs(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint8_t* bases, uint64_t cap_bases, uint64_t* offsets,
                uint64_t* abund, uint8_t* flags, uint64_t cap_unitigs, uint64_t* n_unitigs, uint64_t* n_bases, uint64_t* summary);

/* ---- the links between those unitigs: the edges of the compacted graph (additions, as above).  Everything refers to the
 * unitigs of kmc_unitigs for the same view and range: their numbering, their spelling, the joins after the cycle cuts.
 * UNITIG ENDS.  Unitig u, spelled as the string S_u, has two ends: end 2u + 1, the END end, is the side through which the
 *   reading leaves the last key; end 2u + 0, the START end, is the side of the first key opposite the one it is left
 *   through.  A one-key unitig owns both sides of its key.  Every unitig end is one terminal side state, and every terminal
 *   side state of a solid key is exactly one unitig end.  With rc the reading sense of a key (read on its other strand or
 *   not), its exit side is L if rc, else R; side T of a key is its unitig's END end iff T is the exit side, else the START
 *   end (one-key unitigs included).
 * LINK RECORDS.  For a unitig end with side state a = (x, S): every base c whose bit is set in the S nibble of adj[x], in
 *   ascending c; (y, T) = ext(x, S, c) and its facing side by the rules of kmc_graph.  If (y, T) is a terminal side state
 *   this is one record end(a) -> end(y, T), stored as the uint32_t 2v + e of the target end.  If it is not, no record is
 *   written and summary[5] counts it: that happens only around a palindromic key, so only for even k in a canonical ctx.
 *   Records are directed and every one is kept: a link normally appears twice, once from each end, and nothing is
 *   deduplicated.  A hairpin gives a single record from an end to itself; a cut cycle gives END -> START of the same unitig;
 *   around palindromic keys the record set need not be symmetric.
 * IN GFA TERMS.  Leaving u through its END end reads u+, through its START end u-; arriving at the START end of v reads
 *   v+, at its END end v-.  A record is "L u o1 v o2 (k-1)M": the last k - 1 bases of the oriented u equal the first k - 1 of
 *   the oriented v.  In a forward ctx every END-end record is + + and every START-end record its mirror.
 * Outputs: link_offsets[2 * n_unitigs + 1], uint64_t, indexed by end, link_offsets[0] == 0; link_to[n_links], uint32_t; the
 * records of end i are link_to[link_offsets[i] .. link_offsets[i + 1]).  summary[KMC_LINK_WORDS]: [0] unitigs, [1] records,
 * [2] ends with no record, [3] ends with two or more, [4] records whose target is the source's own unitig, [5] extensions
 * dropped because the target side is not terminal, [6] unitigs with no record at either end, [7] the largest number of
 * records at one end (at most 4).  With g the kmc_graph and t the kmc_unitigs summary of the same range:
 * g[1] + g[2] == [1] + [5] + 2 * (t[2] - t[0]) (every side that is not a unitig end has degree 1).
 * Rules: those of kmc_unitigs (NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no view:
 * KMC_ERR_STATE; a view of 2^31 keys or more: KMC_ERR_CAPACITY; an empty view gives zeros and link_offsets[0] == 0); 2^32
 * records or more: KMC_ERR_CAPACITY.  The table, the view, a partition, a filter result, a set-operation result and the
 * query index are not changed.
 * RELATION TO kmc_unitigs.  A links call counts as a kmc_unitigs* call.  If the ctx still holds the unitigs of this very
 * view and range, and no kmc_graph* call has rewritten the adj words since, it runs the links pass alone; otherwise it
 * computes the unitigs first and keeps that result.  So kmc_unitigs followed by kmc_unitig_links with the same range
 * computes the unitigs once, and the ids in the records are those of the arrays kmc_unitigs handed out (they are in any
 * case: the numbering depends on the view and the range alone).
 * Diagnostic: with KMC_UNITIG_TRACE set, a links call that computes prints "kmc_unitig_links: keys N unitigs U records R
 * unitigs_reused 0|1 links_ms .." to stderr -- a line of its own, behind the kmc_unitigs line if it computed the unitigs
 * too, because that line already calls its partner phase links_ms (tools/measure_links.py reads both). ---- */
#define KMC_LINK_WORDS 8
/* The two arrays in ctx-owned device memory -- uint64_t link_offsets[2 * n_unitigs + 1], uint32_t link_to[n_links] -- valid
 * until the next kmc_unitig_links*, kmc_unitigs* or kmc_graph* call / finalize / reset / destroy (same ordering contract as
 * kmc_export_device).  Every output pointer may be NULL.  Always computes the links pass. */
int kmc_unitig_links_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, const void** d_link_offsets,
                            const void** d_link_to, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* summary);
/* The same, copied to the caller's arrays.  cap_ends counts ENDS: link_offsets has room for cap_ends + 1 entries and needs
 * cap_ends >= 2 * *n_unitigs (not 2 * n_unitigs + 1); link_to has cap_links entries.  Every output pointer may be NULL (an
 * array that is NULL is not copied and its cap not looked at).  *n_unitigs and *n_links are always set; a cap too small for
 * an array that was given -> KMC_ERR_ARG and nothing is copied.  Both arrays NULL is the sizing / summary-only call.  A call
 * whose ctx still holds the links of the last kmc_unitig_links* call for this very view and range copies from that result
 * (the sizing call followed by the call that copies computes once); a finalize, or a kmc_unitigs* or kmc_unitig_links*
 * call that computes, in between makes it compute again. */
int kmc_unitig_links(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t* link_offsets, uint64_t cap_ends,
                     uint32_t* link_to, uint64_t cap_links, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* summary);

/* ---- reads threaded through those unitigs: where every window of a read lies in the compacted graph (additions, as
 * above).  Everything refers to the unitigs of kmc_unitigs for the same view and range min_count..max_count: their
 * numbering, their spelling S_u, their m_u keys.  KMC_MODE_CONTIG only; every k, in a canonical or a forward ctx.
 * WINDOW.  The k bases that start at base j of read r, as the string f: the window kmc_profile counts.  A window is VALID iff
 *   it lies inside the read and holds only upper-case ACGT.
 * PLACED.  A valid window is placed iff x = canon(f) (f itself in a forward ctx) is solid, by the ctx's own key rule and the
 *   range rule of kmc_graph.  x then occurs in exactly one unitig u, at exactly one key position pos in 0..m_u-1, and
 *   S_u[pos : pos+k] is f or its reverse complement.  o = 0 iff f == S_u[pos : pos+k] -- so a palindromic f has o = 0 --
 *   and o = 1 otherwise; in a forward ctx o is always 0.
 * PLACE WORD.  place[offsets[r] + j], a uint64_t: the low 32 bits are uni = 2u + o, the high 32 bits are pos.  A window that
 *   is not placed has uni = KMC_MAP_NONE and pos = 0: the last k-1 positions of a read, every position of a read shorter
 *   than k, invalid windows, windows that are not solid.
 * CONTINUES.  Window j of a read continues window j-1 iff both are placed, their uni is equal, and pos_j == pos_{j-1} + 1
 *   when o = 0, pos_j == pos_{j-1} - 1 when o = 1.  Nothing else counts: a homopolymer read over a one-key circular unitig
 *   does not continue itself, nor does a wrap across a cycle's cut.  The formula is the definition.
 * SEGMENT.  A maximal run of windows of one read, each continuing the one before it, recorded as four uint32_t: start (the
 *   window start relative to the read), len (its number of windows), uni, pos (the position of its first window).  Segments
 *   are listed per read in read order; seg_offsets[n_reads + 1], uint64_t, seg_offsets[0] == 0: the segments of read r are
 *   segs[4 * seg_offsets[r] .. 4 * seg_offsets[r+1]).
 * CROSSING.  A segment whose first window is not the read's first window and whose preceding window is placed: the read
 *   stepped from one unitig end to another without a gap.
 * read_stats[n_reads * KMC_MAP_READ_WORDS], uint32_t: [0] valid windows, [1] placed windows, [2] segments, [3] crossings.
 * support[n_unitigs], uint64_t: placed windows per unitig, on either strand, over the batch.
 * summary[KMC_MAP_WORDS]: [0] reads, [1] valid windows, [2] placed windows, [3] segments, [4] crossings, [5] reads with at
 *   least one valid window, all of them placed, [6] reads with no placed window, [7] the most segments in one read.
 *   [2] equals the sum of support, [3] equals seg_offsets[n_reads].
 * Rules: NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no view: KMC_ERR_STATE (where kmc_export
 * says so); the capacity rules of kmc_unitigs: KMC_ERR_CAPACITY; a read of 2^32 bases or more: KMC_ERR_ARG; 2^32 segments or
 * more in a batch: KMC_ERR_CAPACITY.  n_reads == 0 and an empty view give zeros (an empty view places nothing; its valid
 * windows are still counted).
 * RELATION TO THE OTHER VIEW CALLS.  A map call counts as a kmc_unitigs* call: it reuses the unitigs the ctx holds for this
 * view and range if no kmc_graph* call has rewritten their work arrays (the condition of kmc_unitig_links), otherwise it
 * computes them and keeps them.  It rewrites none of: the unitig arrays, links, a clean result, adj, the view, a partition,
 * a filter or set-operation result, the query index.  Behind the unitigs it keeps one 8-byte word per view row (unitig,
 * position, strand), built once per unitig result and dropped with it.
 * Diagnostic: with KMC_UNITIG_TRACE set, a map call prints "kmc_unitig_map: keys N unitigs U reads R windows W placed P
 * segments S unitigs_reused 0|1 index_ms .. place_ms .. segs_ms .." to stderr (tools/measure_map.py reads it). ---- */
#define KMC_MAP_WORDS 8
#define KMC_MAP_READ_WORDS 4
#define KMC_MAP_NONE 0xFFFFFFFFu
/* The batch in device memory, by the layout and alignment rules of kmc_profile_device (d_bases 16-byte aligned and readable
 * up to the next 16-byte boundary, d_offsets uint64_t[n_reads + 1]).  The results in ctx-owned device arrays -- uint64_t
 * place[n_bases], uint32_t read_stats[n_reads * 4], uint64_t seg_offsets[n_reads + 1], uint32_t segs[4 * n_segs], uint64_t
 * support[n_unitigs] -- valid until the next kmc_unitig_map*, kmc_unitigs* or kmc_graph* call / finalize / reset / destroy
 * (same ordering contract as kmc_export_device).  Every output pointer may be NULL. */
int kmc_unitig_map_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, const void* d_bases, const void* d_offsets,
                          uint64_t n_reads, uint64_t n_bases, const void** d_place, const void** d_read_stats,
                          const void** d_seg_offsets, const void** d_segs, const void** d_support, uint64_t* n_segs,
                          uint64_t* n_unitigs, uint64_t* summary);
/* The same on host buffers (the batch as kmc_profile takes it).  The caller supplies place[offsets[n_reads]],
 * read_stats[n_reads * 4], seg_offsets[n_reads + 1], segs with room for cap_segs records and support with cap_unitigs
 * entries.  *n_segs and *n_unitigs are always set; a cap too small for an array that was given -> KMC_ERR_ARG and nothing
 * is copied; an array that is NULL is not copied and its cap not looked at.  All arrays NULL is the sizing call.  The host
 * form computes on EVERY call -- it cannot recognise a batch it has seen -- so a caller that sizes first maps twice; the
 * device form, which hands out the arrays themselves, needs no sizing call. */
int kmc_unitig_map(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, const uint8_t* bases, const uint64_t* offsets,
                   uint64_t n_reads, uint64_t* place, uint32_t* read_stats, uint64_t* seg_offsets, uint32_t* segs,
                   uint64_t cap_segs, uint64_t* support, uint64_t cap_unitigs, uint64_t* n_segs, uint64_t* n_unitigs,
                   uint64_t* summary);

/* ---- read walks counted per graph element: link support, transits through unitigs, repeat verdicts (additions, as above).
 * Everything refers to the unitigs, the link records and the map result of one view and one range min_count..max_count; a
 * call takes that range and a batch laid out as kmc_unitig_map takes it.  KMC_MODE_CONTIG only; every k, in a canonical or a
 * forward ctx.
 * CROSSING.  kmc_unitig_map's: segment i of read r with i > seg_offsets[r] is a crossing iff segs[i].start ==
 *   segs[i-1].start + segs[i-1].len.  start is relative to the read, so the test alone is not enough across a read boundary:
 *   the first segment of a read is never a crossing.  With uni_a = 2u + o_a of segment i-1 and uni_b = 2v + o_b of segment i,
 *   the read leaves end a = 2u + 1 - o_a and enters end b = 2v + o_b.
 * LINK SUPPORT.  link_support[n_links], uint64_t, indexed like link_to.  For record j of end e with target t = link_to[j] it
 *   holds the number of crossings of the batch with (a, b) == (e, t), plus, if t != e, the number with (a, b) == (t, e): the
 *   same link read on the other strand.  One end never has two records with the same target (distinct extension bases reach
 *   distinct keys, hence distinct ends), so "the record e -> t" is well defined.  A crossing for which neither a -> b nor
 *   b -> a is a record is counted in the summary and nowhere else; that happens only around palindromic keys (even k,
 *   canonical).
 * TRANSIT.  A segment i such that i and i + 1 are both crossings of the same read: the read entered unitig v from somewhere,
 *   ran through it and left it.  o is the orientation bit of segment i; e_in = 2v + o, e_out = 2v + 1 - o; a is the end the
 *   read came from (as above, for crossing i) and b' the end it enters next (for crossing i + 1).  p is the rank (0..3) of
 *   the record e_in -> a among the records of e_in, q the rank of e_out -> b' among those of e_out.  If either record does not
 *   exist the transit is dropped and counted in the summary.  Stored orientation-free: P is the rank at the START end 2v, Q
 *   the rank at the END end 2v + 1: (P, Q) = (p, q) if o == 0, else (q, p).
 * TRANSIT MATRIX.  dS(v) and dE(v) are the record counts of ends 2v and 2v + 1.  transit_offsets[n_unitigs + 1], uint64_t:
 *   transit_offsets[0] == 0 and transit_offsets[v+1] - transit_offsets[v] == dS(v) * dE(v).  transit_count[n_slots], uint64_t:
 *   slot transit_offsets[v] + P * dE(v) + Q holds the number of transits of the batch through v by that pair.  The layout is
 *   dense per unitig, at most 16 slots, and zeros are stored; unitigs with a bare end have no slots.
 * VERDICT.  verdict[n_unitigs], uint8_t, under the parameter min_reads (0 is taken as 1).  KMC_TRANSIT_PLAIN: dS < 2 or
 *   dE < 2.  Every other unitig is a REPEAT, and a slot is supported iff its count is at least min_reads.
 *   KMC_TRANSIT_UNSPANNED: no slot is supported.  KMC_TRANSIT_RESOLVED: every row and every column of the dS x dE matrix has
 *   exactly one supported slot (so dS == dE and the supported slots are a perfect matching; slots below min_reads are noise
 *   and are ignored).  KMC_TRANSIT_AMBIGUOUS: every other repeat.
 * summary[KMC_TRANSIT_WORDS]: [0] crossings, [1] crossings with no record in either direction, [2] records with support 0,
 *   [3] transits stored, [4] transits dropped for a missing record, [5] repeat unitigs, [6] RESOLVED, [7] AMBIGUOUS.  The
 *   formulas are the definition.  [0] equals kmc_unitig_map's summary[4] for the same batch; the sum of transit_count equals
 *   [3].  Where the record set is symmetric -- t -> e is a record whenever e -> t is: every forward ctx and every canonical
 *   ctx of odd k; for even k a canonical set can be asymmetric even when the links summary[5] is 0, because a palindromic key
 *   that is a unitig of its own lists a neighbour at both of its ends and is entered by it through one -- [1] == 0 and
 *   [4] == 0, and the sum of link_support equals 2 * [0] - (crossings with a == b).
 * KMC_TRANSIT_ACCUMULATE (flags bit 0).  Real inputs arrive in many batches.  With the flag the call adds onto the arrays the
 *   ctx still holds from the last transits call of this very view and range: [0], [1], [3], [4] are totals, verdict and [2],
 *   [5]..[7] are recomputed from the totals with this call's min_reads.  No such result held: KMC_ERR_STATE (the first batch
 *   goes without the flag).  The held result is dropped by finalize, reset, destroy and by any call that recomputes the
 *   unitigs or the links -- a kmc_graph* call in between makes the next transits call one of those.  A map, correct, trim,
 *   normalize or profile call in between leaves it alone.
 * RELATION TO THE OTHER VIEW CALLS.  A transits call counts as a kmc_unitig_links call: it reuses the unitigs and links the ctx
 *   still holds for this view and range under the condition of a bubbles call, otherwise it computes them and keeps them.
 *   After that it counts as a kmc_unitig_map_device call on the batch (map arrays handed out earlier are invalid); with no
 *   read or no unitig there is nothing to map and it leaves them alone.  Links first, then map, then the transit passes.  It
 *   rewrites none of: the unitig arrays, link_offsets / link_to, a clean, simplify, components or bubbles result, the view, a
 *   partition, a filter or set-operation result, the query index.
 * Rules: the argument and state errors of kmc_unitig_map (NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count, a bad
 *   batch: KMC_ERR_ARG; no view: KMC_ERR_STATE); unknown flag bits: KMC_ERR_ARG; the capacity rules of the map and links calls,
 *   and 2^32 slots or more: KMC_ERR_CAPACITY.  An empty view gives transit_offsets[0] == 0 and zeros.  n_reads == 0 is legal:
 *   it gives the sizes and the held (ACCUMULATE) or zeroed arrays and adds nothing.
 * Diagnostic: with KMC_UNITIG_TRACE set, a call prints "kmc_unitig_transits: unitigs U records R reads N segments S crossings C
 *   transits T links_reused 0|1 map_ms .. transit_ms .. verdict_ms .." to stderr, behind the lines of what it had to compute
 *   (tools/measure_transits.py reads it).  KMC_TRANSITS_PLAIN in the environment makes every lane add its own 1 instead of
 *   combining equal targets per wave -- a diagnostic for that tool, the result is the same. ---- */
#define KMC_TRANSIT_WORDS 8
#define KMC_TRANSIT_PLAIN 0
#define KMC_TRANSIT_UNSPANNED 1
#define KMC_TRANSIT_RESOLVED 2
#define KMC_TRANSIT_AMBIGUOUS 3
#define KMC_TRANSIT_ACCUMULATE 1u   /* flags bit 0 */
/* The batch in device memory by the rules of kmc_unitig_map_device.  The results in ctx-owned device arrays -- uint64_t
 * link_support[n_links], uint64_t transit_offsets[n_unitigs + 1], uint64_t transit_count[n_slots], uint8_t verdict[n_unitigs]
 * -- valid until the next kmc_unitig_transits*, kmc_unitigs*, kmc_unitig_links* or kmc_graph* call that computes / finalize /
 * reset / destroy (same ordering contract as kmc_export_device).  Every output pointer may be NULL. */
int kmc_unitig_transits_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint32_t flags,
                               const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
                               const void** d_link_support, const void** d_transit_offsets, const void** d_transit_count,
                               const void** d_verdict, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* n_slots,
                               uint64_t* summary);
/* The same on host buffers (the batch as kmc_unitig_map takes it).  link_support has cap_links entries, transit_offsets room
 * for cap_unitigs + 1, transit_count cap_slots, and verdict shares cap_unitigs.  *n_unitigs, *n_links and *n_slots are always
 * set; a cap too small for an array that was given -> KMC_ERR_ARG and nothing is copied; an array that is NULL is not copied
 * and its cap not looked at.  All arrays NULL is the sizing call (kmc_unitig_links plus that call's *n_slots size them as
 * well).  Like kmc_unitig_map's host form it computes on EVERY call: with KMC_TRANSIT_ACCUMULATE size with n_reads == 0, or the
 * batch is added twice. */
int kmc_unitig_transits(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint32_t flags,
                        const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t* link_support,
                        uint64_t cap_links, uint64_t* transit_offsets, uint64_t cap_unitigs, uint64_t* transit_count,
                        uint64_t cap_slots, uint8_t* verdict, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* n_slots,
                        uint64_t* summary);

/* ---- the counted walks acted on: contigs (additions, as above).  Every read-resolved repeat gets one copy per matched way
 * through it, links without support are ignored on request, and the chains of unitigs that remain are spelled out.
 * Everything refers to three results of one view and one range min_count..max_count: the unitigs (S_u, m_u keys, abund), the
 * link records (link_offsets, link_to) and the transits result the ctx holds (link_support, transit_offsets, transit_count).
 * KMC_MODE_CONTIG only; every k, in a canonical or a forward ctx.  Parameters: min_reads (0 is taken as 1) and min_support
 * (0: every record is live).
 * RESOLVED under this call's min_reads: recomputed from transit_count by the VERDICT rule of the transits block; the held
 *   verdict byte is not trusted, it was made with another call's min_reads.  For a resolved unitig v with dS = dE = d,
 *   sigma_v(P) is the one Q whose slot (P, Q) is supported.
 * NODE.  A resolved unitig has d nodes: copy p (0 <= p < d) owns record rank p at its START end 2v and record rank sigma_v(p)
 *   at its END end 2v + 1.  Every other unitig has one node.  node_offsets[u] is the exclusive scan of the copies; the id of
 *   copy p of u is node_offsets[u] + p.  Every node has a START end and an END end.
 * CHOICE of a node end (n, e) with source end s = 2u + e.  The chosen record: for a copy of a resolved unitig the one record
 *   the copy owns at that end, whatever its support; otherwise the live records of s are those with link_support >=
 *   min_support, and if exactly one is live that one is chosen, if not there is no choice.  With t = 2w + f the target of that
 *   record the chosen node end is: if w is not resolved, (its node, f); if w is resolved, let q be the rank of the record
 *   t -> s among all records of t (if it does not exist there is no choice): copy q of w if f is START, copy sigma_w^-1(q) if
 *   f is END, at end f.
 * JOIN.  (n, e) and (n', e') are joined iff each is the other's choice and they are not the same node end -- the mutual rule
 *   of the unitigs; a hairpin record is no join.  Joins are a symmetric matching on node ends, so the nodes fall into simple
 *   paths and simple cycles.
 * CONTIG.  A maximal path or a cycle.  A cycle is cut at the join of the START end of its smallest node, flagged circular,
 *   read from that node in + orientation and spelled without wrap, like a circular unitig.  A path of one node is read +.
 *   Any other path starts at the end node with the smaller id, read + if its unjoined end is START and - if it is END.
 *   Contigs are numbered by their start node, ascending.  The rule does not look at the ctx: in a forward ctx a path that
 *   starts at an END end is spelled on the other strand, and its k-mers are the reverse complements of the table's.
 * Outputs.  path_offsets[n_contigs + 1], uint64_t; path[n_nodes], uint32_t: entries 2u + o, o = 1 where the unitig is read
 *   reverse-complemented.  bases / offsets[n_contigs + 1] in the kmc_add_batch layout: the oriented first unitig, then of
 *   every following one its oriented spelling from base k - 1 on, so a contig has (sum of m_u) + k - 1 bases.
 *   abund[n_contigs], uint64_t: the sum of abund[u] over the path -- a duplicated repeat counts IN FULL in each copy, so the
 *   sum of abund over the contigs exceeds the table's total where something was duplicated.  flags[n_contigs], uint8_t: bit
 *   0 circular.
 * summary[KMC_CONTIG_WORDS]: [0] contigs, [1] nodes, [2] unitigs duplicated, [3] records ignored for support (counted at
 *   the ends of single-copy unitigs), [4] circular contigs, [5] contigs of one node, [6] the most nodes in one contig,
 *   [7] bases.  [1] == path_offsets[n_contigs], [7] == offsets[n_contigs] == (sum over path of m_u) + [0] * (k - 1).
 * With nothing resolved and min_support 0 the joins are those the unitigs already made or refused, and bases, offsets,
 *   abund and flags are those of kmc_unitigs with path[c] == 2c.
 * State.  The call computes nothing it was not given: the ctx must hold the unitigs, the links and a transits result of this
 *   very view and range -- the results, not the work arrays, so a kmc_graph* call in between does not matter as long as the
 *   three are still held -- otherwise KMC_ERR_STATE with a message that names the missing one.  It rewrites none of: the
 *   unitig, link, map and transit arrays, a clean, simplify, components or bubbles result, the view, a partition, a filter
 *   or set-operation result, the query index.  The held contig result is keyed by view, range, min_reads and min_support;
 *   it is dropped by any transits call (the counts changed), by anything that drops the links, and by finalize, reset and
 *   destroy.
 * Rules: NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no view: KMC_ERR_STATE; 2^31 nodes or
 *   more, or 2^32 keys or more over the paths: KMC_ERR_CAPACITY.  An empty view gives zeros and offsets[0] ==
 *   path_offsets[0] == 0.
 * Diagnostic: with KMC_UNITIG_TRACE set, a call that computes prints "kmc_unitig_contigs: unitigs U nodes N contigs C bases B
 *   rounds R choice_ms .. rank_ms .. layout_ms .. emit_ms .." to stderr (tools/measure_contigs.py reads it). ---- */
#define KMC_CONTIG_WORDS 8
/* The results in ctx-owned device arrays -- uint8_t bases[n_bases] (readable to the next 16-byte boundary, as
 * kmc_add_batch_device asks), uint64_t offsets[n_contigs + 1], uint64_t path_offsets[n_contigs + 1], uint32_t path[n_nodes],
 * uint64_t abund[n_contigs], uint8_t flags[n_contigs] -- valid until the next kmc_unitig_contigs* call that computes, a
 * transits call, anything that drops the links / finalize / reset / destroy (same ordering contract as kmc_export_device).
 * Computes on every call.  Every output pointer may be NULL. */
int kmc_unitig_contigs_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint64_t min_support,
                              const void** d_bases, const void** d_offsets, const void** d_path_offsets, const void** d_path,
                              const void** d_abund, const void** d_flags, uint64_t* n_contigs, uint64_t* n_nodes,
                              uint64_t* n_bases, uint64_t* summary);
/* The same on host buffers.  bases has cap_bases entries; offsets and path_offsets have room for cap_contigs + 1, abund and
 * flags for cap_contigs; path has cap_nodes.  *n_contigs, *n_nodes and *n_bases are always set; a cap too small for an array
 * that was given -> KMC_ERR_ARG and nothing is copied; an array that is NULL is not copied and its cap not looked at.  All
 * arrays NULL is the sizing call; a sizing call followed by the copy call computes once, as for kmc_unitig_links. */
int kmc_unitig_contigs(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t min_reads, uint64_t min_support,
                       uint8_t* bases, uint64_t cap_bases, uint64_t* offsets, uint64_t* path_offsets, uint64_t* abund,
                       uint8_t* flags, uint64_t cap_contigs, uint32_t* path, uint64_t cap_nodes, uint64_t* n_contigs,
                       uint64_t* n_nodes, uint64_t* n_bases, uint64_t* summary);

/* ---- pair evidence: which two unitig ends the mates of a pair connect, across how many bases, and the insert sizes
 * (additions, as above).  The paired counterpart of kmc_unitig_transits: it counts and reports, exactly and
 * deterministically; it joins nothing.  Everything refers to the unitigs of one view and one range min_count..max_count --
 * S_u, m_u keys, L_u = m_u + k - 1 bases -- and to the segments kmc_unitig_map gives for the batch, each (start, len, uni =
 * 2u + o, pos).  KMC_MODE_CONTIG only; every k, in a canonical or a forward ctx.  The formula is the definition.
 * PAIR.  Reads 2i (mate A) and 2i + 1 (mate B) are pair i, n_pairs = n_reads / 2, as KMC_TRIM_PAIR_* and KMC_NORM_PAIRED
 *   take them; an odd n_reads is KMC_ERR_ARG.  The library model is forward / reverse: the mates come from opposite strands of
 *   one fragment and each is read from its own 5' end towards the other.  RF (mate-pair) and FF libraries are left out on
 *   purpose: reverse-complement the mates before the call.
 * ANCHOR of a mate.  The longest of its segments (greatest len), of equally long ones the one with the greatest segment
 *   index.  A mate with no segment has no anchor.  With the anchor (s, len, 2u + o, pos):
 *     out end  e = 2u + 1 - o, the end of u the mate points at;
 *     reach    = s + (o ? pos + 1 : m_u - pos) + k - 1, the bases from the mate's first base to that end of u, extrapolated
 *              along u (64-bit arithmetic).
 * CLASS of a pair, one byte.  KMC_PAIR_UNPLACED: a mate has no anchor.  KMC_PAIR_SPAN: u_A != u_B.  u_A == u_B and o_A != o_B:
 *   with R = reach_A + reach_B, KMC_PAIR_PROPER iff R > L_u, and its insert size is F = R - L_u; KMC_PAIR_EVERTED otherwise.
 *   (With x_A = pos_A - s_A and x_B = pos_B + k - 1 + s_B as base coordinates on S_u -- the first base of the mate read
 *   along S_u, the last base of the mate read against it -- F = x_B - x_A + 1.)  KMC_PAIR_SAME_STRAND: u_A == u_B and o_A ==
 *   o_B.  No special case is made for circular unitigs, hairpins or palindromes.
 * PAIR RECORD.  The SPAN pairs grouped by the unordered pair of their out ends, (a, b) = (min(e_A, e_B), max(e_A, e_B)),
 *   listed in ascending (a, b).  One record holds count, the sum of R = reach_A + reach_B, min R and max R.  With a library
 *   insert size F the estimated gap between the two ends is F - sum / count (host arithmetic); for two ends joined by a link
 *   record it is -(k - 1) for error-free reads.
 * Outputs.  Per pair: pair_class[n_pairs], uint8_t; pair_ends[2 * n_pairs], uint32_t: e_A, e_B, KMC_MAP_NONE for a mate
 *   without an anchor; pair_value[n_pairs], uint64_t: R for SPAN, F for PROPER, else 0.  Per record: rec_ends[2 * n_records],
 *   uint32_t: a, b; rec_count, rec_sum, rec_min, rec_max [n_records], uint64_t.  insert_hist[n_bins], uint64_t: bin
 *   min(F, n_bins - 1) over the PROPER pairs (F >= 1, so bin 0 stays 0); 2 <= n_bins <= 2^20.
 * summary[KMC_PAIR_WORDS]: [0] pairs, [1] UNPLACED, [2] SPAN, [3] PROPER, [4] EVERTED, [5] SAME_STRAND, [6] records, [7] the
 *   sum of F over the PROPER pairs.  Identities, checked by the host on every call: [0] == [1] + [2] + [3] + [4] + [5]; the sum
 *   of rec_count == [2]; the sum of insert_hist == [3]; [6] == n_records <= [2].
 * KMC_PAIR_ACCUMULATE (flags bit 0).  Every output except the three per-pair arrays is additive, min / max included.  With
 *   the flag the call gives exactly what one call on the concatenation of this batch behind all batches accumulated so far
 *   would give, with the same n_bins; the per-pair arrays describe this batch alone.  The held result is keyed by view, range
 *   and n_bins; no such result held: KMC_ERR_STATE (the first batch goes without the flag).  It is dropped where the transits
 *   result is dropped -- finalize, reset, destroy, anything that recomputes the unitigs (a kmc_graph* call in between makes
 *   the next pairs call one of those).  n_reads == 0 is legal and returns the held (ACCUMULATE) or zeroed result.
 * RELATION TO THE OTHER VIEW CALLS.  A pairs call counts as a kmc_unitig_map_device call on the batch, as a transits call does
 *   (map arrays handed out earlier are invalid): it reuses the unitigs the ctx holds under the same condition, otherwise it
 *   computes them and keeps them.  It does not need the links.  It rewrites none of: the unitig, link, transit or contig
 *   results, a clean, simplify, components or bubbles result, the view, a partition, a filter or set-operation result, the
 *   query index -- a pairs call between kmc_unitig_transits and kmc_unitig_contigs leaves the contigs call working, and a
 *   transits call leaves a held pairs result alone.  The records are grouped by the library's own radix sort; it works in
 *   scratch of its own and touches neither the view nor the runs the view is made of.
 * Rules: the argument, state and capacity errors of kmc_unitig_transits; an odd n_reads, unknown flag bits, n_bins outside
 *   2..2^20: KMC_ERR_ARG; 2^32 records or more, a view of more than 2^30 unitigs (two ends share one 64-bit sort key below the
 *   all-ones filler), 2^32 pairs and held records or more in one call: KMC_ERR_CAPACITY.  An empty view gives zeros and every
 *   pair is UNPLACED.
 * Diagnostic: with KMC_UNITIG_TRACE set, a call prints "kmc_unitig_pairs: unitigs U pairs N span S proper P records R
 *   unitigs_reused 0|1 map_ms .. anchor_ms .. sort_ms .. reduce_ms .." to stderr, behind the lines of what it had to compute
 *   (anchor_ms: the anchor and the pair pass; tools/measure_pairs.py reads it).  KMC_PAIRS_PLAIN in the environment, read per
 *   call, makes every lane of the reduce pass issue its own atomics instead of combining per workgroup -- a diagnostic for
 *   that tool, the result is the same.  KMC_PAIRS_GRID=N, read per call, caps the workgroups of the pair and reduce passes (a
 *   test sends a small batch through many rounds of one workgroup with it); the result is the same. ---- */
#define KMC_PAIR_WORDS 8
#define KMC_PAIR_UNPLACED 0
#define KMC_PAIR_SPAN 1
#define KMC_PAIR_PROPER 2
#define KMC_PAIR_EVERTED 3
#define KMC_PAIR_SAME_STRAND 4
#define KMC_PAIR_ACCUMULATE 1u   /* flags bit 0 */
/* The batch in device memory by the rules of kmc_unitig_map_device.  The results in ctx-owned device arrays -- uint8_t
 * pair_class[n_pairs], uint32_t pair_ends[2 * n_pairs], uint64_t pair_value[n_pairs], uint32_t rec_ends[2 * n_records],
 * uint64_t rec_count / rec_sum / rec_min / rec_max [n_records], uint64_t insert_hist[n_bins] -- valid until the next
 * kmc_unitig_pairs* call / finalize / reset / destroy (same ordering contract as kmc_export_device).  Every output pointer
 * may be NULL. */
int kmc_unitig_pairs_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t n_bins, uint32_t flags,
                            const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
                            const void** d_pair_class, const void** d_pair_ends, const void** d_pair_value,
                            const void** d_rec_ends, const void** d_rec_count, const void** d_rec_sum, const void** d_rec_min,
                            const void** d_rec_max, const void** d_insert_hist, uint64_t* n_pairs, uint64_t* n_records,
                            uint64_t* summary);
/* The same on host buffers (the batch as kmc_unitig_map takes it).  The three per-pair arrays share cap_pairs, the five
 * record arrays cap_records (rec_ends has room for 2 * cap_records), insert_hist has cap_bins entries.  *n_pairs and
 * *n_records are always set; a cap too small for an array that was given -> KMC_ERR_ARG and nothing is copied; an array that
 * is NULL is not copied and its cap not looked at.  No sizing call is needed: n_pairs == n_reads / 2, n_records <= n_pairs
 * plus the records held (ACCUMULATE), and insert_hist has n_bins entries.  Like kmc_unitig_map's host form it computes on
 * EVERY call: with KMC_PAIR_ACCUMULATE a second call on the same batch adds it twice. */
int kmc_unitig_pairs(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t n_bins, uint32_t flags,
                     const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint8_t* pair_class, uint32_t* pair_ends,
                     uint64_t* pair_value, uint64_t cap_pairs, uint32_t* rec_ends, uint64_t* rec_count, uint64_t* rec_sum,
                     uint64_t* rec_min, uint64_t* rec_max, uint64_t cap_records, uint64_t* insert_hist, uint64_t cap_bins,
                     uint64_t* n_pairs, uint64_t* n_records, uint64_t* summary);

/* ---- reads corrected against the table: substitution errors repaired from the solid keys (additions, as above).
 * KMC_MODE_CONTIG only; every k, in a canonical or a forward ctx.  Reads the sorted view of the last kmc_finalize (a view
 * queued by kmc_finalize_async counts as one).  A key is SOLID by the range rule of kmc_graph (min_count, max_count, 0 = no
 * upper bound).  The batch is NOT counted.
 * WINDOW.  For a read R of L bases, window j (0 <= j <= L - k) is f = R[j : j+k].  It is VALID iff f holds only upper-case
 *   ACGT (kmc_profile's rule), WEAK iff valid and canon(f) is not solid (canon: the ctx's own key rule), STRONG iff valid and
 *   solid.
 * WEAK RUN.  A maximal run [a, b] of consecutive weak windows of one read, n = b - a + 1.  Its left border is START if
 *   a == 0, SOLID if window a - 1 is strong, INVALID otherwise; its right border is END if b == L - k, SOLID if window b + 1
 *   is strong, INVALID otherwise.
 * CANDIDATE.  A weak run is a candidate with suspect position p (relative to the read) iff one of:
 *     kind 0, KMC_CORRECT_INTERIOR: left SOLID, right SOLID, n == k; p = b.
 *     kind 1, KMC_CORRECT_HEAD:     left START, right SOLID, n <= k; p = b.
 *     kind 2, KMC_CORRECT_TAIL:     left SOLID, right END,   n <= k; p = a + k - 1.
 *   Nothing else is: not a run with an INVALID border, not an interior run of any other length (two errors closer than k, an
 *   error whose windows are partly solid by chance), not a read that is weak from end to end.  In all three kinds the
 *   windows a..b are exactly the windows of the read that contain p.
 * ACCEPTED.  For each base c of ACGT other than R[p]: c is accepted iff every window a..b of R with R[p] replaced by c is
 *   strong.  The accepted mask has bit code(c) set per accepted base.  Exactly one accepted base: the candidate is CORRECTED
 *   and the corrected read carries c at p.  None: it stays.  Two or three: it is AMBIGUOUS and stays.  The formula is the
 *   definition; no count-weighted choice is made.
 * INDEPENDENCE.  Two candidates of one read have suspect positions more than k - 1 apart, and no candidate's windows contain
 *   another candidate's suspect position.  So testing every candidate against the read as it came gives the same result as
 *   testing them in any order on the partly corrected read; a correction turns exactly its n windows strong and changes no
 *   other window; correcting the corrected batch again corrects nothing.
 * Outputs.  bases[n_bases]: the batch with the corrected positions replaced; every other byte is copied as given, N and
 *   lower case included; the offsets are the caller's own.  cand_offsets[n_reads + 1], uint64_t, [0] == 0, and
 *   cands[4 * n_cands], uint32_t: one record per candidate, in read order and by position within a read:
 *   [0] p, [1] old ASCII byte | new ASCII byte << 8 (new == old unless corrected) | kind << 16 | accepted mask << 24, [2] a,
 *   [3] n.  read_stats[n_reads * KMC_CORRECT_READ_WORDS], uint32_t: [0] valid windows, [1] weak windows, [2] candidates,
 *   [3] corrected.  summary[KMC_CORRECT_WORDS]: [0] reads, [1] valid windows, [2] weak windows, [3] weak runs, [4] candidates,
 *   [5] corrected, [6] ambiguous, [7] weak windows left = [2] minus the sum of n over the corrected candidates.
 *   [4] == cand_offsets[n_reads], and [7] equals word [2] of a second call on the corrected batch.
 * Rules: NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no view: KMC_ERR_STATE (where kmc_export
 * says so); a view of 2^32 keys or more: KMC_ERR_CAPACITY (the index's rule); a read of 2^32 bases or more: KMC_ERR_ARG; 2^32
 * candidates or more: KMC_ERR_CAPACITY.  n_reads == 0 gives zeros.  An empty view gives no candidate and the batch back as
 * it came; its valid windows are all weak and are counted.
 * What the call changes: it builds or reuses the query index.  It rewrites none of: the view, a partition, a filter or
 * set-operation result, adj, the unitigs, links, a clean result, a map result.  Left out on purpose: insertions and
 * deletions, an N replaced by a base, two errors within k of each other, a choice among ambiguous bases by count.
 * Diagnostic: with KMC_UNITIG_TRACE set, a call prints "kmc_correct: keys N reads R windows W weak X runs U cands C fixed F
 * mark_ms .. runs_ms .. try_ms .." to stderr (tools/measure_correct.py reads it). ---- */
#define KMC_CORRECT_WORDS 8
#define KMC_CORRECT_READ_WORDS 4
#define KMC_CORRECT_INTERIOR 0u
#define KMC_CORRECT_HEAD 1u
#define KMC_CORRECT_TAIL 2u
/* The batch in device memory, by the layout and alignment rules of kmc_profile_device.  The results in ctx-owned device
 * arrays -- uint8_t corrected[n_bases], uint32_t read_stats[n_reads * 4], uint64_t cand_offsets[n_reads + 1], uint32_t
 * cands[4 * n_cands] -- valid until the next kmc_correct* call / finalize / reset / destroy (same ordering contract as
 * kmc_export_device: the call has finished when it returns).  d_corrected obeys the alignment and padding rule of
 * kmc_add_batch_device: with the caller's d_offsets it goes straight into kmc_add_batch_device, kmc_profile_device or
 * kmc_unitig_map_device of this or another ctx on this device, and back into kmc_correct_device.  Every output pointer may
 * be NULL. */
int kmc_correct_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, const void* d_bases, const void* d_offsets,
                       uint64_t n_reads, uint64_t n_bases, const void** d_corrected, const void** d_read_stats,
                       const void** d_cand_offsets, const void** d_cands, uint64_t* n_cands, uint64_t* summary);
/* The same on host buffers (the batch as kmc_profile takes it).  The caller supplies out_bases[offsets[n_reads]],
 * read_stats[n_reads * 4], cand_offsets[n_reads + 1] and cands with room for cap_cands records.  *n_cands is always set; a
 * cap too small for cands when it is given -> KMC_ERR_ARG and nothing is written; an array that is NULL is not copied and
 * has no cap.  All arrays NULL is the sizing call.  The host form computes on EVERY call. */
int kmc_correct(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, const uint8_t* bases, const uint64_t* offsets,
                uint64_t n_reads, uint8_t* out_bases, uint32_t* read_stats, uint64_t* cand_offsets, uint32_t* cands,
                uint64_t cap_cands, uint64_t* n_cands, uint64_t* summary);

/* ---- reads trimmed and filtered by their solid k-mers (additions, as above): which reads, and which part of each, the
 * table supports -- quality trimming behind kmc_correct, decontamination (INVERT against a contaminant's table), baiting.
 * KMC_MODE_CONTIG only; every k, in a canonical or a forward ctx.  Reads the sorted view of the last kmc_finalize (a view
 * queued by kmc_finalize_async counts as one).  The batch is NOT counted.  The formula is the definition.
 * WINDOW, VALID, STRONG, WEAK.  Exactly as in the kmc_correct block: window j of a read R of L bases is R[j : j+k], 0 <= j <=
 *   L - k; valid iff it holds only upper-case ACGT; strong iff valid and canon(f) is solid by the range rule of kmc_graph
 *   (min_count, max_count, 0 = no upper bound); weak iff valid and not strong.  V = valid windows of the read, S = strong
 *   windows.
 * STRONG RUN.  A maximal set of consecutive window indices of one read that are all strong; an invalid or weak window, or
 *   the read's end, ends it.  F / E = index of the first / last strong window of the read.  (B, N) = start and length in
 *   windows of the longest strong run; of several longest runs, the one with the smallest start.
 * SPAN, by mode, as (start, len) in bases relative to the read:
 *     KMC_TRIM_NONE (0):    (0, L).
 *     KMC_TRIM_ENDS (1):    (F, E - F + k) if S > 0, else (0, 0).  Weak and invalid windows inside stay.
 *     KMC_TRIM_LONGEST (2): (B, N + k - 1) if S > 0, else (0, 0).  Every window of the span is strong.
 * PASS.  A read passes iff all of: S >= min_strong; S * 1000 >= (uint64_t)min_permille * V, as plain 64-bit products;
 *   len >= min_len; mode == KMC_TRIM_NONE || S > 0.  A read with no valid window passes only if min_strong == 0, min_len <= L
 *   and the mode is NONE: no special case is made.
 * PAIRS.  flags & KMC_TRIM_PAIR_BOTH or flags & KMC_TRIM_PAIR_EITHER: reads 2i and 2i + 1 are mates.  Giving both flags, or
 *   an odd n_reads, is KMC_ERR_ARG.  The pair's verdict is the AND (BOTH) or the OR (EITHER) of its mates' PASS, and both
 *   mates get it.  Without a pair flag a read's verdict is its own PASS.
 * INVERT.  flags & KMC_TRIM_INVERT: a read is emitted iff its verdict is false.  This requires mode == KMC_TRIM_NONE,
 *   otherwise KMC_ERR_ARG.  Without the flag a read is emitted iff its verdict is true.
 * Outputs.  out_bases: the spans of the emitted reads, concatenated in read order, bytes copied as given (lower case and N
 *   inside an ENDS span included).  out_offsets[n_out + 1], uint64_t, [0] == 0.  origin[n_out], uint64_t: the source read
 *   of each emitted read.  read_stats[n_reads * KMC_TRIM_READ_WORDS], uint32_t, for EVERY read, emitted or not: [0] V,
 *   [1] S, [2] span start, [3] span len.  verdict[n_reads], uint8_t: bit 0 (KMC_TRIM_PASS) = the read's own PASS, bit 1
 *   (KMC_TRIM_EMITTED) = emitted.  summary[KMC_TRIM_WORDS]: [0] reads, [1] valid windows, [2] strong windows, [3] reads whose
 *   own PASS is true, [4] reads emitted (= n_out), [5] bases emitted (= out_offsets[n_out]), [6] emitted reads whose span is
 *   shorter than the read, [7] the bases of the emitted reads before trimming.  Bases cut off the emitted reads: [7] - [5].
 * Identities.  Mode NONE with min_strong = min_permille = min_len = 0 and no flags returns the batch as it came: same bytes,
 *   same offsets, origin[i] == i.  The same arguments with INVERT emit nothing.  A second call with the same arguments on the
 *   output of a LONGEST or ENDS call (min_len 0) returns that output unchanged; after LONGEST its summary has [1] == [2].
 *   For every read, words [0], [1] equal words [0] and [0] - [1] of kmc_correct's read_stats for the same range.  With
 *   max_count == 0, words [0], [1] equal words [0], [1] of kmc_profile's read_stats with the same min_count.
 * Rules: NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count, an unknown mode or flag bit, min_permille > 1000, the
 * flag combinations above, a read of 2^32 bases or more: KMC_ERR_ARG; no view: KMC_ERR_STATE (where kmc_export says so); a
 * view of 2^32 keys or more: KMC_ERR_CAPACITY (the index's rule); a batch of 2^31 reads or 2^32 bases or more in one call:
 * KMC_ERR_CAPACITY (the positions among the emitted reads and bases are scanned as 32-bit words; split the batch).
 * n_reads == 0 gives zeros and out_offsets[0] == 0.  An empty view makes nothing strong.
 * What the call changes: it builds or reuses the query index.  It rewrites none of: the view, a partition, a filter or
 * set-operation result, adj, the unitigs, links, a clean / simplify / components result, a map result, and the arrays a
 * kmc_correct* call handed out.
 * Diagnostic: with KMC_UNITIG_TRACE set, a call prints "kmc_trim: keys N reads R windows W strong S passed P emitted E bases
 * B mark_ms .. reduce_ms .. layout_ms .. gather_ms .." to stderr (tools/measure_trim.py reads it). ---- */
#define KMC_TRIM_WORDS 8
#define KMC_TRIM_READ_WORDS 4
#define KMC_TRIM_NONE 0
#define KMC_TRIM_ENDS 1
#define KMC_TRIM_LONGEST 2
#define KMC_TRIM_INVERT 1u
#define KMC_TRIM_PAIR_BOTH 2u
#define KMC_TRIM_PAIR_EITHER 4u
#define KMC_TRIM_PASS 1u      /* verdict bit 0 */
#define KMC_TRIM_EMITTED 2u   /* verdict bit 1 */
/* The batch in device memory, by the layout and alignment rules of kmc_profile_device.  The results in ctx-owned device
 * arrays -- uint8_t out_bases[n_out_bases], uint64_t out_offsets[n_out + 1], uint64_t origin[n_out], uint32_t read_stats[n_reads
 * * 4], uint8_t verdict[n_reads] -- valid until the next kmc_trim* call / finalize / reset / destroy (the contract of
 * kmc_correct_device: the call has finished when it returns).  d_out_bases is 16-byte aligned and readable to the next 16-byte
 * boundary past the last base (those bytes are zero): with d_out_offsets it goes straight into kmc_add_batch_device,
 * kmc_profile_device, kmc_unitig_map_device, kmc_correct_device and back into kmc_trim_device, of this or another ctx on the
 * device.  A caller may hand the last call's own d_out_bases / d_out_offsets back in: the ctx double-buffers the two arrays
 * (a call writes the pair the call before it did not), so the result of the call BEFORE the last one is gone.  Every output
 * pointer may be NULL. */
int kmc_trim_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, int mode, uint32_t flags, uint64_t min_strong,
                    uint32_t min_permille, uint64_t min_len, const void* d_bases, const void* d_offsets, uint64_t n_reads,
                    uint64_t n_bases, const void** d_out_bases, const void** d_out_offsets, const void** d_origin,
                    const void** d_read_stats, const void** d_verdict, uint64_t* n_out, uint64_t* n_out_bases,
                    uint64_t* summary);
/* The same on host buffers (the batch as kmc_profile takes it).  The caller supplies out_bases with room for cap_bases
 * bytes, out_offsets with room for cap_reads + 1 entries, origin for cap_reads, read_stats[n_reads * 4] and verdict[n_reads].
 * *n_out and *n_out_bases are always set; a cap too small for an array that was given -> KMC_ERR_ARG and nothing is copied;
 * an array that is NULL is not copied and its cap not looked at.  All arrays NULL is the sizing call.  The host form computes
 * on EVERY call. */
int kmc_trim(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, int mode, uint32_t flags, uint64_t min_strong,
             uint32_t min_permille, uint64_t min_len, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads,
             uint8_t* out_bases, uint64_t cap_bases, uint64_t* out_offsets, uint64_t* origin, uint64_t cap_reads,
             uint32_t* read_stats, uint8_t* verdict, uint64_t* n_out, uint64_t* n_out_bases, uint64_t* summary);

/* ---- read depth normalised (additions, as above): every read gets a depth, a percentile of the counts of its k-mers; reads
 * of over-covered regions are sampled down to a target depth and reads below a floor depth are dropped (digital
 * normalisation in its static, two-pass form: the table is given and each read is judged on its own, so the result does not
 * depend on the order of the reads).  KMC_MODE_CONTIG only; every k, in a canonical or a forward ctx.  Reads the sorted view
 * of the last kmc_finalize (a view queued by kmc_finalize_async counts as one).  The batch is NOT counted.  The formula is
 * the definition.
 * WINDOW, VALID.  Exactly kmc_profile's: window j of a read R of L bases is R[j : j+k], 0 <= j <= L - k; valid iff it holds
 *   only upper-case ACGT.  c(j) is the entry window_count of kmc_profile: the view's count of canon(f) (of f in a forward
 *   ctx), 0 if absent, saturated at 0xFFFFFFFF.  There is no count range.  V = valid windows of the read.
 * DEPTH.  The counts of the V valid windows sorted ascending, c_(0) <= ... <= c_(V-1); q = ((V - 1) * permille) / 1000 by
 *   64-bit integer division, permille in 0..1000; the read's own depth is d_r = c_(q), and d_r = 0 if V == 0.  permille 0 is
 *   the minimum, 1000 the maximum, 500 the lower median.
 * UNIT.  Without KMC_NORM_PAIRED the unit of read r is g = r and D = d_r.  With it reads 2i and 2i + 1 are mates, g = r >> 1
 *   and D = min(d_2i, d_2i+1); an odd n_reads is KMC_ERR_ARG.
 * DRAW.  All arithmetic mod 2^64: x = seed + (g + 1) * 0x9E3779B97F4A7C15; x ^= x >> 30; x *= 0xBF58476D1CE4E5B9;
 *   x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31; u = ((x >> 32) * D) >> 32 -- 0 when D == 0, else in 0..D-1.
 * LOW, DEEP.  LOW iff D < min_depth.  DEEP iff not LOW, target != 0 and D > target.
 * KEEP, EMITTED.  KEEP iff not LOW and (not DEEP or u < target): a DEEP unit survives with probability target / D.  Both
 *   mates of a pair get their unit's verdict.  EMITTED is KEEP; with KMC_NORM_INVERT it is not KEEP.  target == 0 samples
 *   nothing down, min_depth == 0 drops nothing.
 * Outputs.  out_bases: the emitted reads whole, concatenated in read order, bytes as given.  out_offsets[n_out + 1],
 *   uint64_t, [0] == 0.  origin[n_out], uint64_t: the source read of each emitted read.  read_stats[n_reads *
 *   KMC_NORMALIZE_READ_WORDS], uint32_t, for EVERY read, emitted or not: [0] V, [1] d_r, [2] D, [3] u.  verdict[n_reads],
 *   uint8_t: bit 0 KMC_NORM_KEEP, bit 1 KMC_NORM_EMITTED, bit 2 KMC_NORM_LOW, bit 3 KMC_NORM_DEEP.
 *   summary[KMC_NORMALIZE_WORDS]: [0] reads, [1] valid windows, [2] reads emitted (= n_out), [3] bases emitted (=
 *   out_offsets[n_out]), [4] LOW reads, [5] DEEP reads, [6] DEEP reads that are kept, [7] the sum of d_r.  Without INVERT
 *   [2] == [0] - [4] - [5] + [6].
 * Identities.  For one seed, the units kept at target T1 are a subset of those kept at T2 > T1 (u does not depend on the
 *   target).  permille 0 and 1000 give d_r = min(kmc_profile's read_stats [2] and [3], 0xFFFFFFFF), and word [0] equals
 *   kmc_profile's [0].  target 0, min_depth 0 and no flags return the batch as it came: same bytes, same offsets, origin[i]
 *   == i.  The same arguments with INVERT emit nothing.
 * Rules: NULL ctx, KMC_MODE_LR, permille > 1000, an unknown flag bit, an odd n_reads with PAIRED, a read of 2^32 bases or
 * more, the ctx's own last kmc_normalize* output arrays handed in as the input (the call would read what it writes; the
 * outputs of kmc_trim* and kmc_correct* are fine as input, and this call's are fine as input to them): KMC_ERR_ARG; no view:
 * KMC_ERR_STATE (where kmc_export says so); a view of 2^32 keys or more: KMC_ERR_CAPACITY (the index's rule); a batch of 2^31
 * reads or 2^32 bases or more in one call: KMC_ERR_CAPACITY (kmc_trim's rule).  target or min_depth above 2^32 are plain
 * 64-bit comparisons.  n_reads == 0 gives zeros and out_offsets[0] == 0.  An empty view makes every count 0.
 * What the call changes: it builds or reuses the query index.  It rewrites none of: the view, a partition, a filter or
 * set-operation result, adj, the unitigs, links, a clean / simplify / components / bubbles result, a map result, and the
 * arrays a kmc_correct* or kmc_trim* call handed out.
 * Diagnostic: with KMC_UNITIG_TRACE set, a call prints "kmc_normalize: keys N reads R windows W emitted E bases B low L deep
 * D kept K profile_ms .. select_ms .. layout_ms .. gather_ms .." to stderr (tools/measure_normalize.py reads it). ---- */
#define KMC_NORMALIZE_WORDS 8
#define KMC_NORMALIZE_READ_WORDS 4
#define KMC_NORM_PAIRED 1u
#define KMC_NORM_INVERT 2u
#define KMC_NORM_KEEP 1u      /* verdict bit 0 */
#define KMC_NORM_EMITTED 2u   /* verdict bit 1 */
#define KMC_NORM_LOW 4u       /* verdict bit 2 */
#define KMC_NORM_DEEP 8u      /* verdict bit 3 */
/* The batch in device memory, by the layout and alignment rules of kmc_profile_device.  The results in ctx-owned device
 * arrays -- uint8_t out_bases[n_out_bases], uint64_t out_offsets[n_out + 1], uint64_t origin[n_out], uint32_t read_stats[n_reads
 * * 4], uint8_t verdict[n_reads] -- valid until the next kmc_normalize* call / finalize / reset / destroy (the contract of
 * kmc_trim_device: the call has finished when it returns).  d_out_bases is 16-byte aligned and readable to the next 16-byte
 * boundary past the last base (those bytes are zero): with d_out_offsets it goes straight into kmc_add_batch_device,
 * kmc_correct_device, kmc_trim_device and kmc_unitig_map_device, of this or another ctx on the device -- but not back into
 * kmc_normalize* of this ctx (above).  Every output pointer may be NULL. */
int kmc_normalize_device(kmc_ctx* ctx, uint32_t permille, uint64_t target, uint64_t min_depth, uint64_t seed, uint32_t flags,
                         const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void** d_out_bases,
                         const void** d_out_offsets, const void** d_origin, const void** d_read_stats, const void** d_verdict,
                         uint64_t* n_out, uint64_t* n_out_bases, uint64_t* summary);
/* The same on host buffers (the batch as kmc_profile takes it), by the cap conventions of kmc_trim: out_bases with room for
 * cap_bases bytes, out_offsets for cap_reads + 1 entries, origin for cap_reads, read_stats[n_reads * 4] and verdict[n_reads].
 * *n_out and *n_out_bases are always set; a cap too small for an array that was given -> KMC_ERR_ARG and nothing is copied;
 * an array that is NULL is not copied and its cap not looked at.  All arrays NULL is the sizing call.  The host form computes
 * on EVERY call. */
int kmc_normalize(kmc_ctx* ctx, uint32_t permille, uint64_t target, uint64_t min_depth, uint64_t seed, uint32_t flags,
                  const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint8_t* out_bases, uint64_t cap_bases,
                  uint64_t* out_offsets, uint64_t* origin, uint64_t cap_reads, uint32_t* read_stats, uint8_t* verdict,
                  uint64_t* n_out, uint64_t* n_out_bases, uint64_t* summary);

/* ---- the compacted graph cleaned: tips clipped, islands dropped (additions, as above).  Everything refers to the unitigs
 * and the link records of kmc_unitigs / kmc_unitig_links for the same view and range min_count..max_count.  For unitig u:
 * m_u = offsets[u + 1] - offsets[u] - (k - 1) its number of keys, A_u = abund[u], rec(e) the record list of end e.
 * ISLAND.  u is an island iff it is not circular, rec(2u) and rec(2u + 1) are both empty and m_u <= max_island_keys.
 * TIP CANDIDATE.  u is a tip candidate iff it is not circular, m_u <= max_tip_keys, exactly one of its ends has no record and
 *   the other, the attached end a, has exactly one.  (A stem that leads into a fork has two or more records at its attached
 *   end: it is no candidate.)
 * TIP.  Let t be the one record of a.  The siblings of u are the records s of rec(t) with s != a and s >> 1 != u.  u is a tip
 *   iff it is a candidate and some sibling's unitig w = s >> 1 dominates it: w is not a tip candidate, or w is one and beats u
 *   -- by higher mean abundance, compared exactly as the 128-bit products A_w * m_u > A_u * m_w; on a tie by m_w > m_u; on
 *   a tie by w < u.  So of the dead-end arms that compete at one junction exactly the best survives, and beside any sibling
 *   that is not a candidate (a long one, or one that continues) every candidate goes.  Hairpins get no special case (a
 *   record from an end to itself gives no sibling), nor do the dropped or asymmetric records around palindromic keys: the
 *   formula is the definition.
 * VERDICT.  verdict[u], a uint8_t: KMC_CLEAN_KEEP, KMC_CLEAN_TIP or KMC_CLEAN_ISLAND.  (An island is never a candidate.)
 * KEPT TABLE.  The solid keys whose unitig's verdict is KEEP, in view order, with their counts: key_hi (NULL / zeros when
 *   keys fit one word), key_lo, count -- the shape of a view, as kmc_filter_device gives it, so that it goes straight into
 *   another ctx through kmc_merge_pairs_device.
 * summary[KMC_CLEAN_WORDS]: [0] unitigs, [1] tips, [2] islands, [3] keys kept, [4] keys of tips, [5] keys of islands, [6] tip
 *   candidates (those that survive included), [7] the sum of the counts of the kept keys.  With t the kmc_unitigs summary of
 *   the same range: [3] + [4] + [5] == t[2].
 * LIMITS.  max_tip_keys == 0 clips nothing, max_island_keys == 0 drops nothing; with both 0 the kept table equals
 *   kmc_export_filtered of the range.  A limit of 2^31 or more is unlimited.
 * Rules: those of kmc_unitig_links (NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no view:
 * KMC_ERR_STATE; the capacity rules of the links: KMC_ERR_CAPACITY; an empty view gives zeros).
 * RELATION TO THE OTHER VIEW CALLS.  A clean call counts as a kmc_unitig_links* call: it reuses the unitigs and links the ctx
 * still holds for this view and range (and whose work arrays no kmc_graph* call has rewritten), otherwise it computes them
 * and keeps them.  It rewrites neither of them, nor adj, nor the view, a partition, a filter result, a set-operation result
 * or the query index: the arrays a preceding links or unitigs call of this range handed out stay valid.
 * Diagnostic: with KMC_UNITIG_TRACE set, a clean pass prints "kmc_unitig_clean: keys N unitigs U tips T islands I kept K
 * clean_ms .." to stderr, behind the lines of the unitigs and links it had to compute (tools/measure_clean.py reads it). ---- */
#define KMC_CLEAN_WORDS 8
#define KMC_CLEAN_KEEP 0
#define KMC_CLEAN_TIP 1
#define KMC_CLEAN_ISLAND 2
/* The kept table and uint8_t verdict[n_unitigs] in ctx-owned device memory, valid until the next kmc_unitig_clean*,
 * kmc_unitig_links*, kmc_unitigs* or kmc_graph* call / finalize / reset / destroy (same ordering contract as
 * kmc_export_device).  Every output pointer may be NULL.  Always computes the clean pass. */
int kmc_unitig_clean_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                            const void** d_key_hi, const void** d_key_lo, const void** d_count, const void** d_verdict,
                            uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary);
/* The same, copied to the caller's arrays: key_hi / key_lo / count of cap_keys entries each, verdict of cap_unitigs bytes.
 * Every output pointer may be NULL (an array that is NULL is not copied and its cap not looked at).  *n_kept and *n_unitigs
 * are always set; a cap too small for an array that was given -> KMC_ERR_ARG and nothing is copied.  All arrays NULL is the
 * sizing / summary-only call.  A call whose ctx still holds the clean result for this very view, range and pair of limits
 * copies from it: the sizing call followed by the call that copies computes once. */
int kmc_unitig_clean(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                     uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap_keys, uint8_t* verdict, uint64_t cap_unitigs,
                     uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary);
/* One step of a cleaning round: kmc_unitig_clean_device on src, then the kept pairs merged into dst as
 * kmc_merge_pairs_device(dst, ...) would; the merge has finished when the call returns.  dst must differ from src and agree
 * with it in device, mode, k and canonical (KMC_ERR_ARG otherwise; errors are reported on src).  dst is left un-finalized,
 * so several sources can be merged; kmc_finalize(dst) then gives the cleaned table, on which the next round's kmc_unitigs /
 * kmc_unitig_links / kmc_unitig_clean_into run.  summary may be NULL. */
int kmc_unitig_clean_into(kmc_ctx* src, kmc_ctx* dst, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys,
                          uint64_t max_island_keys, uint64_t* summary);

/* ---- the same with simple bubbles popped: the third shape a sequencing error leaves (additions, as above).  A substitution
 * in the interior of a read gives k erroneous keys: one short unitig that leaves the true path at a fork and rejoins it k keys
 * later, beside the true arm of the same length.  It has one record at each end, so it is neither a tip nor an island.
 * Everything refers to the unitigs and the link records of kmc_unitigs / kmc_unitig_links for the same view and range; m_u,
 * A_u and rec(e) are as in the clean block above.
 * BUBBLE CANDIDATE.  u is a bubble candidate iff it is not circular, m_u <= max_bubble_keys, rec(2u) has exactly one record
 *   p and rec(2u + 1) exactly one record q, p != q, p >> 1 != u and q >> 1 != u.  ends(u) = {p, q}.
 * PARALLEL.  Candidates u and w != u are parallel iff ends(w) == ends(u) as sets.  Orientation may differ: in a canonical
 *   ctx the other arm is often spelled the other way round.
 * BUBBLE.  u is a bubble iff it is a candidate and, among the records s of rec(p) -- p the one record of u's START end --
 *   with s >> 1 != u, some unitig w = s >> 1 is a candidate parallel to u that beats u, in the order of the tip rule:
 *   A_w * m_u > A_u * m_w as 128-bit products; on a tie m_w > m_u; on a tie w < u.  The order is strict, so two parallel
 *   arms are never both popped; where the records are symmetric exactly the best of the parallel arms survives and the two
 *   junctions stay connected.  Around palindromic keys (even k, canonical) records can be missing or asymmetric; no special
 *   case is made: the formula is the definition, as for tips.  Arms of more than one unitig (nested or complex bubbles) are
 *   not looked for.
 * TIPS AND ISLANDS are decided exactly as by kmc_unitig_clean.  The three classes exclude one another by their record
 *   counts (0 + 0, 0 + 1, 1 + 1).  A bubble arm is not a tip candidate, so it dominates a tip at its junction as before,
 *   also when the same pass pops the arm: its surviving parallel arm stays.
 * VERDICT.  KMC_CLEAN_KEEP, KMC_CLEAN_TIP, KMC_CLEAN_ISLAND or KMC_CLEAN_BUBBLE.  The kept table is that of the clean block.
 * ABUNDANCE.  The counts of a popped arm's keys are NOT added to the surviving arm: they leave the table and summary[11]
 *   says how much left.
 * summary[KMC_SIMPLIFY_WORDS]: [0..7] as in KMC_CLEAN_WORDS, [3] and [7] counting what is kept after all three removals;
 *   [8] bubbles popped, [9] keys of popped bubbles, [10] bubble candidates (those that survive included), [11] the sum of the
 *   counts of the popped bubbles' keys.  With t the kmc_unitigs summary of the same range: [3] + [4] + [5] + [9] == t[2].
 * LIMITS.  max_bubble_keys == 0 pops nothing: verdicts, kept table and words [0..7] are those of kmc_unitig_clean with the
 *   same arguments and words [8..11] are 0.  2^31 or more is unlimited.
 * Rules, ordering contract, pointer lifetimes, NULL-able outputs and the sizing call are those of kmc_unitig_clean*.
 * RELATION TO THE OTHER VIEW CALLS.  A simplify call counts as a clean call: it reuses the unitigs and links under the same
 *   conditions, writes the buffers a clean call writes (so it ends the validity of a clean result's pointers and the other
 *   way round) and rewrites nothing else.  The result a ctx holds is keyed by view, range and the three limits, a clean call
 *   having bubble limit 0: kmc_unitig_clean behind a simplify with a non-zero bubble limit computes again, and the other
 *   way round; a simplify with limit 0 and a clean with the same arguments share one result.
 * Diagnostic: with KMC_UNITIG_TRACE set, a simplify pass that computes prints "kmc_unitig_simplify: keys N unitigs U tips T
 * islands I bubbles B kept K clean_ms .." to stderr, behind the lines of the unitigs and links it had to compute
 * (tools/measure_simplify.py reads it); a kmc_unitig_clean* call prints its own line as before. ---- */
#define KMC_SIMPLIFY_WORDS 12
#define KMC_CLEAN_BUBBLE 3
/* kmc_unitig_clean_device with the bubble rule.  Always computes the pass. */
int kmc_unitig_simplify_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                               uint64_t max_bubble_keys, const void** d_key_hi, const void** d_key_lo, const void** d_count,
                               const void** d_verdict, uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary);
/* kmc_unitig_clean with the bubble rule; the sizing call followed by the call that copies computes once. */
int kmc_unitig_simplify(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys, uint64_t max_island_keys,
                        uint64_t max_bubble_keys, uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap_keys,
                        uint8_t* verdict, uint64_t cap_unitigs, uint64_t* n_kept, uint64_t* n_unitigs, uint64_t* summary);
/* kmc_unitig_clean_into with the bubble rule: one step of a round that also pops bubbles. */
int kmc_unitig_simplify_into(kmc_ctx* src, kmc_ctx* dst, uint64_t min_count, uint64_t max_count, uint64_t max_tip_keys,
                             uint64_t max_island_keys, uint64_t max_bubble_keys, uint64_t* summary);

/* ---- the compacted graph as a whole: its connected components labelled, the small ones dropped (additions, as above).
 * Everything refers to the unitigs and the link records of kmc_unitigs / kmc_unitig_links for the same view and range
 * min_count..max_count; m_u, A_u and rec(e) are as in the clean block above.
 * ADJACENT.  Unitigs u and v are adjacent iff some record of an end of u targets an end of v, or some record of an end of v
 *   targets an end of u.  The union matters: around palindromic keys (even k, canonical) the record set need not be
 *   symmetric.  No special case is made: the formula is the definition.  Self records (hairpins, the END -> START record of a
 *   cut cycle) relate a unitig to itself and change nothing.
 * COMPONENT.  An equivalence class of the reflexive-transitive closure of ADJACENT.  Every unitig is in exactly one.
 * ROOT.  The smallest unitig id of a component.
 * NUMBERING.  Components are numbered 0..n_comps-1 by ascending ROOT, so component 0 contains unitig 0.  The numbering
 *   depends on the view and the range alone.
 * Per component c: unitigs(c), keys(c) = the sum of m_u, abund(c) = the sum of A_u (exact, uint64_t).
 * SMALL.  c is small iff keys(c) <= max_component_keys.  max_component_keys == 0 makes nothing small, 2^31 or more is
 *   unlimited (the rule of the clean limits).  There is NO exemption for circular unitigs -- the one place where this rule
 *   differs from ISLAND: a one-unitig cycle of m <= max_component_keys keys is a small component, while kmc_unitig_clean
 *   never calls a circular unitig an island.
 * VERDICT.  verdict[u], a uint8_t: KMC_CLEAN_KEEP, or KMC_CLEAN_COMPONENT when u's component is small.
 * KEPT TABLE.  The solid keys whose unitig's verdict is KEEP, in view order, with their counts: the shape of a view, exactly
 *   as kmc_unitig_clean* hands one out, so that it goes straight into kmc_merge_pairs_device.
 * Outputs.  comp_of[n_unitigs], uint32_t: the component number of each unitig.  comp_stats[n_comps *
 *   KMC_COMPONENT_STAT_WORDS], uint64_t, four words per component: [0] ROOT, [1] unitigs, [2] keys, [3] abund.
 *   verdict[n_unitigs].  The kept table.
 * summary[KMC_COMPONENT_WORDS]: [0] unitigs, [1] components, [2] components of one unitig, [3] the most keys in one
 *   component, [4] the most unitigs in one component, [5] small components, [6] keys kept, [7] the sum of the counts of the
 *   kept keys.
 * IDENTITIES.  With t the kmc_unitigs summary and l the kmc_unitig_links summary of the same range: the sum of
 *   comp_stats[.][1] == [0] == t[0]; the sum of comp_stats[.][2] == t[2]; the sum of comp_stats[.][3] == t[7]; [2] >= l[6]
 *   (an isolated unitig is a one-unitig component, and so is a unitig that has only self records).  With limit 0 the kept
 *   table equals kmc_export_filtered of the range.  With limits (tip 0, island N) every unitig kmc_unitig_clean calls ISLAND
 *   is KMC_CLEAN_COMPONENT here with max_component_keys = N.
 * Rules: those of kmc_unitig_links (NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no view:
 * KMC_ERR_STATE; the capacity rules of the links: KMC_ERR_CAPACITY).  An empty view or a range with nothing solid gives zeros
 * and n_comps == 0.
 * RELATION TO THE OTHER VIEW CALLS.  A components call counts as a kmc_unitig_links* call: it reuses the unitigs and links the
 *   ctx still holds for this view and range under the condition of a clean call, otherwise it computes them and keeps them.  It
 *   rewrites none of: the unitig arrays, the links, adj, the view, a partition, a filter or set-operation result, the query
 *   index, a map or correct result, a clean / simplify result -- in particular the pointers a preceding
 *   kmc_unitig_simplify_device handed out stay valid and unchanged.  Its own result is keyed by view, range and limit;
 *   whatever drops the links (a kmc_unitigs* or kmc_unitig_links_device call, any call that computes them again) drops it.
 * Diagnostic: with KMC_UNITIG_TRACE set, a components pass that computes prints "kmc_unitig_components: keys N unitigs U
 * records R components C small S kept K rounds T label_ms .. number_ms .. stats_ms .. keep_ms .." to stderr, behind the lines
 * of the unitigs and links it had to compute (tools/measure_components.py reads it); T counts the label rounds up to and
 * including the one that hooked nothing. ---- */
#define KMC_COMPONENT_WORDS 8
#define KMC_COMPONENT_STAT_WORDS 4
#define KMC_CLEAN_COMPONENT 4
/* comp_of, comp_stats, verdict and the kept table in ctx-owned device memory, valid until the next kmc_unitig_components*,
 * kmc_unitig_links*, kmc_unitigs* or kmc_graph* call / finalize / reset / destroy (same ordering contract as
 * kmc_export_device; a clean or simplify call shares scratch with this one but leaves these arrays alone).  Every output
 * pointer may be NULL.  Always computes the components pass. */
int kmc_unitig_components_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t max_component_keys,
                                 const void** d_comp_of, const void** d_comp_stats, const void** d_verdict,
                                 const void** d_key_hi, const void** d_key_lo, const void** d_count,
                                 uint64_t* n_comps, uint64_t* n_unitigs, uint64_t* n_kept, uint64_t* summary);
/* The same, copied to the caller's arrays: comp_of (uint32_t) and verdict of cap_unitigs entries each, comp_stats of
 * cap_comps * KMC_COMPONENT_STAT_WORDS words, key_hi / key_lo / count of cap_keys entries each.  Every output pointer may be
 * NULL (an array that is NULL is not copied and its cap not looked at).  *n_comps, *n_unitigs and *n_kept are always set; a
 * cap too small for an array that was given -> KMC_ERR_ARG and nothing is copied.  All arrays NULL is the sizing /
 * summary-only call.  A call whose ctx still holds the result for this very view, range and limit copies from it: the sizing
 * call followed by the call that copies computes once. */
int kmc_unitig_components(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t max_component_keys,
                          uint32_t* comp_of, uint8_t* verdict, uint64_t cap_unitigs, uint64_t* comp_stats, uint64_t cap_comps,
                          uint64_t* key_hi, uint64_t* key_lo, uint64_t* count, uint64_t cap_keys,
                          uint64_t* n_comps, uint64_t* n_unitigs, uint64_t* n_kept, uint64_t* summary);
/* kmc_unitig_clean_into with this rule: kmc_unitig_components_device on src, then the kept pairs merged into dst as
 * kmc_merge_pairs_device(dst, ...) would; the merge has finished when the call returns.  dst must differ from src and agree
 * with it in device, mode, k and canonical (KMC_ERR_ARG otherwise; errors are reported on src); dst is left un-finalized.
 * summary may be NULL. */
int kmc_unitig_components_into(kmc_ctx* src, kmc_ctx* dst, uint64_t min_count, uint64_t max_count,
                               uint64_t max_component_keys, uint64_t* summary);

/* ---- the bubbles of the compacted graph reported, not popped: variant records (additions, as above).  Everything refers to
 * the unitigs and the link records of kmc_unitigs / kmc_unitig_links for the same view and range min_count..max_count.  m_u,
 * A_u and rec(e) are those of the clean block; BUBBLE CANDIDATE, ends(u) = {p, q}, PARALLEL and the order "w beats u" (128-bit
 * products, then keys, then the smaller id) are exactly those of the simplify block, with max_bubble_keys as the candidate
 * limit.
 * MAJOR ARM.  For a candidate u, with p the one record of its START end, let P(u) be the unitigs w = s >> 1 of the records s
 *   of rec(p) with w != u that are candidates parallel to u.  If P(u) is not empty, major(u) is its greatest element under
 *   "beats" (the order is strict and total, so that is one unitig).  u is CALLED iff major(u) beats u.  So u is called exactly
 *   when kmc_unitig_simplify with the same three arguments and tip and island limits 0 gives it KMC_CLEAN_BUBBLE, and the number
 *   of records equals that call's summary[8].  Around palindromic keys the formula is the definition, as everywhere else.
 * ORIENTED ARMS.  U = S_u.  With w = major(u): W = S_w if the one record of w's START end equals p; otherwise W is the reverse
 *   complement of S_w and the record's flag bit KMC_BUBBLE_REVERSED is set.  By the overlap property of the links U and W
 *   begin with the same k - 1 bases and end with the same k - 1 bases.
 * DIFFERENCE.  lcp is the length of the longest common prefix of U and W.  lcs is the length of their longest common suffix,
 *   capped at min(|U|, |W|) - lcp: prefix first, so the two never overlap in the shorter arm.  The alleles are
 *   U[lcp : |U| - lcs] and W[lcp : |W| - lcs].  mism is the Hamming distance of U and W if |U| == |W|, else 0.
 * KIND.  KMC_BUBBLE_SUBST: |U| == |W| and mism == 1.  KMC_BUBBLE_INDEL: exactly one allele is empty.  KMC_BUBBLE_COMPLEX:
 *   everything else (two substitutions closer than k give mism == 2 and alleles of length 2).
 * RECORD.  KMC_BUBBLE_RECORD_WORDS = 8 uint32_t words per called unitig, in ascending u: [0] u, [1] w = major(u), [2] p,
 *   [3] q, [4] lcp, [5] lcs, [6] the kind in bits 0-1 (KMC_BUBBLE_KIND) and KMC_BUBBLE_REVERSED in bit 2, [7] mism.  Allele
 *   lengths, arm lengths and abundances follow from the unitig arrays.
 * summary[KMC_BUBBLE_WORDS]: [0] unitigs, [1] records, [2] bubble candidates (kmc_unitig_simplify's [10]), [3] substitutions,
 *   [4] indels, [5] complex, [6] records with KMC_BUBBLE_REVERSED, [7] the sum of m_u over the called arms
 *   (kmc_unitig_simplify's [9] with tip and island limits 0).  [3] + [4] + [5] == [1].
 * LIMITS.  max_bubble_keys == 0 gives no records (and no candidates).  max_bubble_keys of 2^31 or more is KMC_ERR_ARG here --
 *   not "unlimited" as for the clean calls -- because the positions in a record are uint32_t.
 * Rules: otherwise those of kmc_unitig_links (NULL ctx, KMC_MODE_LR, a non-zero max_count below min_count: KMC_ERR_ARG; no
 * view: KMC_ERR_STATE; the capacity rules of the links: KMC_ERR_CAPACITY; an empty view gives zeros).
 * RELATION TO THE OTHER VIEW CALLS.  A bubbles call counts as a kmc_unitig_links* call: it reuses the unitigs and links the
 *   ctx still holds for this view and range under the condition of a clean call, otherwise it computes them and keeps them.
 *   It writes a result of its own and nothing else: the unitig arrays, the links, adj, the view, a partition, a filter or
 *   set-operation result, the query index, a map or correct result and a clean / simplify / components result -- their
 *   pointers included -- stay valid and unchanged.  Its own result is keyed by view, range and limit; whatever drops the links
 *   (a kmc_unitigs* or kmc_unitig_links_device call, any call that computes them again) drops it.
 * Diagnostic: with KMC_UNITIG_TRACE set, a bubbles pass that computes prints "kmc_unitig_bubbles: keys N unitigs U candidates C
 * records R subst S indel I complex X reversed V pair_ms .. diff_ms .." to stderr, behind the lines of the unitigs and links it
 * had to compute (tools/measure_bubbles.py reads it): pair_ms the pair pass and the scan, diff_ms the records. ---- */
#define KMC_BUBBLE_WORDS 8
#define KMC_BUBBLE_RECORD_WORDS 8
#define KMC_BUBBLE_SUBST 0u
#define KMC_BUBBLE_INDEL 1u
#define KMC_BUBBLE_COMPLEX 2u
#define KMC_BUBBLE_KIND(flags) ((flags) & 3u)
#define KMC_BUBBLE_REVERSED 4u      /* bit 2 of word [6] */
/* uint32_t records[n_records * KMC_BUBBLE_RECORD_WORDS] in ctx-owned device memory, valid until the next kmc_unitig_bubbles*,
 * kmc_unitig_links*, kmc_unitigs* or kmc_graph* call / finalize / reset / destroy (same ordering contract as
 * kmc_export_device).  Every output pointer may be NULL.  Always computes the bubbles pass. */
int kmc_unitig_bubbles_device(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t max_bubble_keys,
                              const void** d_records, uint64_t* n_records, uint64_t* n_unitigs, uint64_t* summary);
/* The same, copied to the caller's array of cap_records * KMC_BUBBLE_RECORD_WORDS words.  Every output pointer may be NULL
 * (records NULL: nothing is copied and its cap not looked at).  *n_records and *n_unitigs are always set; a cap too small for
 * an array that was given -> KMC_ERR_ARG and nothing is copied.  records NULL is the sizing / summary-only call.  A call
 * whose ctx still holds the result for this very view, range and limit copies from it: the sizing call followed by the call
 * that copies computes once. */
int kmc_unitig_bubbles(kmc_ctx* ctx, uint64_t min_count, uint64_t max_count, uint64_t max_bubble_keys, uint32_t* records,
                       uint64_t cap_records, uint64_t* n_records, uint64_t* n_unitigs, uint64_t* summary);

/* Multi-GPU reduce for small tables: ONE fixed-size all-gather instead of size exchange +
 * all-to-all (the reduce of main.rs:87's grouping across GPUs; for the generator's input a table is
 * a few thousand keys, so the exchange is latency-bound and every host synchronisation counts).
 * A slab holds up to slab_entries (key,count) pairs behind an 8-word header; kmc_slab_words gives
 * its size in 64-bit words for this ctx's key width.  kmc_pack_slab_device writes this ctx's table
 * into d_slab -- the sorted view after kmc_finalize, otherwise straight from the live table
 * (unsorted; no finalize and no host synchronisation needed first) -- or marks the slab "oversize"
 * when the table has more than slab_entries keys (live table: also more than 1048576, the length of its list of claimed slots).  kmc_merge_slabs_device adds, from n_slabs consecutive slabs (the all-gather
 * result), every pair with kmc_owner_of(key, n_parts) == my_part; oversize slabs are skipped and
 * counted in kmc_stats.n_slabs_skipped at the next kmc_finalize (the caller then moves those
 * tables with kmc_partition_device + all-to-all + kmc_merge_pairs_device).  Both calls are
 * asynchronous on the ctx stream and never synchronise with the host. */
uint64_t kmc_slab_words(const kmc_ctx* ctx, uint64_t slab_entries);
int kmc_pack_slab_device(kmc_ctx* ctx, void* d_slab, uint64_t slab_entries);
int kmc_merge_slabs_device(kmc_ctx* ctx, const void* d_slabs, uint32_t n_slabs, uint64_t slab_entries,
                           uint32_t my_part, uint32_t n_parts);

/* Drop what the ctx has learned about its data source (the walk kernel's memo of the input's
 * de Bruijn graph structure and the launch planner's new-keys-per-k-mer history); kmc_reset keeps
 * both because later batches of the same source profit from them.  Counts are not affected. */
/* Wait for everything queued on the ctx and read its device counters: brings kmc_stats up to date
 * (n_kmers, kernel_ms_*) and lets the launch planner learn from the batch just counted -- what
 * kmc_finalize does on the way, for callers that reset a ctx without finalizing it (multi-GPU
 * reduce: the live table is packed and shipped, only the owner's table is finalized). */
int kmc_poll(kmc_ctx* ctx);

/* Wait until everything queued on the ctx's stream has finished (nothing else: no counters are read).
 * For callers that hand buffers written by ctx kernels to another stream or library (the RCCL
 * all-gather of a slab packed on a ctx-owned stream). */
int kmc_sync(kmc_ctx* ctx);

/* How KMC_ALGO_WALK cuts a read of read_len bases into pieces of at most 416 bases that overlap by
 * k-1 (every window of the read lies in exactly one piece): the number of pieces, and, for the
 * first `cap`, their [start, end) within the read.  Pure host arithmetic (no GPU needed). */
uint64_t kmc_read_pieces(uint64_t read_len, int k, uint64_t* starts, uint64_t* ends, uint64_t cap);

#define KMC_FORGET_MEMO 1     /* the walk kernel's memo snapshot */
#define KMC_FORGET_HISTORY 2  /* the launch planner's history (and the AUTO algorithm choice) */
int kmc_forget_source(kmc_ctx* ctx, int what);

int kmc_get_stats(const kmc_ctx* ctx, kmc_stats* out);

/* Convenience used by the CLI: parse `path` on the host (restating the reader the reference
 * uses, main.rs:45-46,59-62), feed batches, finalize.  Results via kmc_export. */
int kmc_count_file(kmc_ctx* ctx, const char* path, uint64_t* n_distinct, uint64_t* n_total);

/* The same on several GPUs of this process (the CLI's --gpus N): ctxs[0..n_ctx) are distinct
 * contexts with the same k / mode / canonical, normally one per GPU; chunks of the file go
 * round-robin to them and the tables are reduced into ctxs[0] (peer copies + kmc_merge_pairs_device),
 * which holds the result (kmc_export).  Scaling runs use one process per GPU and RCCL instead
 * (k-mer-count_amd/distributed.py). */
int kmc_count_file_multi(kmc_ctx** ctxs, uint32_t n_ctx, const char* path, uint64_t* n_distinct, uint64_t* n_total);

/* Host FASTA reader on its own (library-owned buffers; free with kmc_free_reads). */
typedef struct kmc_reads {
    uint8_t*  bases;
    uint64_t* offsets;
    uint64_t  n_reads;
    uint64_t  n_bases;
    uint64_t  max_read_len;
} kmc_reads;
int  kmc_parse_fasta(const char* path, kmc_reads* out, char* errbuf, size_t errbuf_len);
void kmc_free_reads(kmc_reads* r);

/* Streaming form of the reader: the file is handed out in chunks of about chunk_bytes of FASTA text
 * (0 = 256 MiB), each ending at a record boundary, parsed by worker threads.  out->bases/offsets
 * point into the stream's own buffers and stay valid until the next call on the stream (do NOT
 * pass them to kmc_free_reads).  *eof is set to 1 with the last chunk.  This is what a host
 * program (the Rust main() of INTEGRATION.md) feeds to kmc_add_batch chunk by chunk;
 * kmc_count_file uses the same reader internally and overlaps parsing with upload and counting.
 * Extension (not in the reference): a file whose first byte is '@' is read as
 * four-line FASTQ and only its sequence lines are handed on. */
typedef struct kmc_fasta_stream kmc_fasta_stream;
int  kmc_fasta_stream_open(const char* path, uint64_t chunk_bytes, kmc_fasta_stream** out, char* errbuf, size_t errbuf_len);
int  kmc_fasta_stream_next(kmc_fasta_stream* s, kmc_reads* out, int* eof, char* errbuf, size_t errbuf_len);
void kmc_fasta_stream_close(kmc_fasta_stream* s);

/* Decode a key into klen ASCII characters (no terminator). */
void kmc_decode_key(uint64_t key_hi, uint64_t key_lo, int klen, char* out);

/* ---- synthetic input: seeded, size-parameterised re-creation of the distribution of
 * random_fasta_generator.py:5-15 (pool of `pool` random lines of `line_len` bases; each record
 * = `lines_per_record` lines drawn uniformly from the pool; pool == 0: every line fresh random).
 * Counter-based PRNG, so any record range can be generated independently and identically on
 * host and device. ---- */
typedef struct kmc_synth {
    uint64_t seed;
    uint32_t pool;             /* 10 in the reference (:5) */
    uint32_t line_len;         /* 80 (:6) */
    uint32_t lines_per_record; /* 5 (:13) */
    uint32_t reserved;
} kmc_synth;

/* Number of records whose FASTA text (header ">dummy_sequence_NNN Nth record\n", :11-12, plus
 * lines) first reaches `file_bytes` bytes; also the exact byte size of that text. */
uint64_t kmc_synth_records_for_bytes(const kmc_synth* s, uint64_t file_bytes, uint64_t* exact_bytes);
/* Parsed form of records [first, first+n): bases (n*lines*line_len bytes) and offsets[n+1]. */
int kmc_synth_reads_host(const kmc_synth* s, uint64_t first_record, uint64_t n_records,
                         uint8_t* bases, uint64_t* offsets);
int kmc_synth_reads_device(const kmc_synth* s, uint64_t first_record, uint64_t n_records,
                           void* d_bases, void* d_offsets, int device, void* stream);
/* FASTA text of records [first, first+n) appended to `FILE_ptr` (a FILE*). */
int kmc_synth_write_fasta(const kmc_synth* s, uint64_t first_record, uint64_t n_records, void* FILE_ptr);

/* ---- measurement aid: the streaming-read rate this GPU actually reaches, so that a kernel's
 * fraction of the HBM roofline can be quoted against the measured peak beside the nominal 8 TB/s.  A plain
 * read-only kernel (non-temporal 16-byte loads of [d_buf, d_buf + n_bytes), xor-reduced; no product code) is
 * launched iters times after one warm-up, bracketed by one hipEvent pair on `stream`; *ms_avg = time per launch.
 * shape: 0 = the walk kernel's grid (one 1024-thread workgroup per CU), 1 = 8 x 256 threads per CU,
 * 2 = 2 x 1024 per CU, 3 = 4 x 512 per CU.  *xor_out (may be NULL) receives the checksum that keeps the loads alive. */
int kmc_read_peak_device(const void* d_buf, uint64_t n_bytes, int device, void* stream, int shape, int iters,
                         double* ms_avg, uint64_t* xor_out);

#ifdef __cplusplus
}
#endif
#endif /* KMC_H */
