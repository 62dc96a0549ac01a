// kmc_ctx.hip.h -- what kmc_api.hip and kmc_views.hip share (internal, not installed): the context behind include/kmc.h,
// its device buffers, error reporting, and what the view layer calls of the counting side.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <exception>
#include <new>
#include <vector>

#include "../../include/kmc.h"
#include "kmc_device.hip.h"
#include "kmc_mem.hip.h"

struct MsdCtl;   // kmc_msd.hip.h

// Every buffer below is owned by its type (kmc_mem.hip.h): a ctx, a Table, a Run or a local that goes away frees what it
// holds, and none of them can be copied.
using DevBuf = Dev<void>;   // an untyped buffer that ensure() sizes: read through .p with the cast of the use

// a (key, count) table the library hands out or keeps for itself; hi is allocated for two-word keys only
struct KeyBufs { DevBuf hi, lo, cnt; };

struct Table {
    Dev<u64> hi, lo, cnt, mid;  // (mid: three-word keys of the (k+16)-mer table, k >= 48)
    u64 cap = 0;
    void reset() { *this = Table{}; }
};

// "The result this ctx still holds": the view generation and the count range a derived result (unitigs, links, the clean
// pass) was computed for.  A stage asks holds() before it computes again, keep()s when its result is complete, and
// drop()s before it rewrites the result arrays.
struct ResultKey {
    u64 gen = ~0ull, min = 0, max = 0;
    bool holds(u64 view_gen, u64 min_count, u64 max_count) const { return gen == view_gen && min == min_count && max == max_count; }
    void keep(u64 view_gen, u64 min_count, u64 max_count) { gen = view_gen; min = min_count; max = max_count; }
    void drop() { gen = ~0ull; }
};

// The stream is a base of kmc_ctx so that it outlives every buffer: members are destroyed before bases, so the last free
// has happened when an owned stream is destroyed.  (kmc_destroy synchronises it before the first.)
struct CtxStream {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    CtxStream() = default;
    CtxStream(const CtxStream&) = delete;
    CtxStream& operator=(const CtxStream&) = delete;
    ~CtxStream() { if (own_stream && stream) (void)hipStreamDestroy(stream); }
};

struct kmc_ctx : CtxStream {
    kmc_config cfg{};
    int KW = 1;     // key words
    int klen = 0;   // characters per key (k, or 54 in LR mode)
    char err[512] = {0};

    Table tab;
    Dev<u64> d_counters;            // 2 * KMC_CTR_N u64: [count table | (k+16)-mer table]
    Pin<u64> h_counters;            // pinned mirror
    Dev<u64> occ_list;              // first KMC_OCC_LIST_CAP claimed slots (fast finalize of small tables)
    Dev<u64> occ_key_lo, occ_key_hi;   // ... and their keys, dense (GTable::occ_key_*)
    Dev<u32> fin_rank;              // ticket counter of kmc_small_finalize_kernel (zero between launches)
    Pin<u64> h_pub;                 // pinned, 2 * KMC_CTR_N: where kmc_small_finalize_kernel publishes its outcome + the counters.  Its
                                    // own block: a kernel queued by kmc_finalize_async may publish after the host has reset or
                                    // polled h_counters; poll_fin copies what the awaited launch published into h_counters
    u64* d_mirror = nullptr;        // h_pub as the device sees it (an alias, not an owner)
    Pin<u64> h_restore;             // pinned: the counters to put back when a drained table is filled again (undrain)
    // planner invariant (kmc_stats.n_planner_stale): every kernel queued OUTSIDE the count launches' own accounting that
    // changes the table -- the (k+16)-mer unfold, merges -- bumps table_epoch; a poll records the epoch it has seen; a
    // risky launch must save a table whose counters were polled at the current epoch
    u64 table_epoch = 0, polled_epoch = 0;
    u64 fin_seq = 0;                // number of the last kmc_small_finalize_kernel launch (the kernel publishes it with its result)
    bool async_fin = false;         // kmc_finalize_async: a finalize is queued whose outcome the host has not looked at yet
    bool drained = false;           // the last kmc_finalize emptied the table into the sorted view (kmc_small_finalize_kernel):
                                    // table and device counters are as after kmc_reset, h_counters hold the true totals
    Dev<u64> spill_hi, spill_lo, spill_cnt;
    u64 spill_cap = 0;

    // staging for host batches
    DevBuf st_bases, st_offsets;
    // sorted view
    KeyBufs o, t, p;   // the small-table finalize's view / the merge sort's input / kmc_partition_device's result
    DevBuf t_idx0;     // the partition's per-owner counters, then cursors
    u64 n_sorted = 0;
    bool sorted_valid = false;
    // walk-kernel workspace
    DevBuf walk_ws;
    DevBuf vr_reads, vr_cnt, vr_pos;  // pieces of long reads for the walk kernel: [starts | ends], per-read counts and their scan
    DevBuf walk_memo;  // two shared memo snapshots + dense counters, kept across launches (kmc_walk.hip.h)
    int memo_parity = 0;  // snapshot slot the next walk launch reads
    bool walk_no_uniform = false;  // KMC_WALK_NO_UNIFORM=1 at kmc_create: uniform-length batches take the ragged kernels too
    bool walk_ws_clean = false;  // workspace header + dense counters are zero (left so by kmc_walk_tail_kernel)
    // The rank plan of the walk path (kmc_walk_plan.hip.h), kept next to the memo and forgotten with it: item -> view row, the
    // rows' keys.  plan_valid: built (queued) for the memo as it stands; plan_stale: its last launch met a counter without a
    // row -- the next suitable finalize rebuilds it, while plan_budget lasts.  plan_src_ok: the table the next finalize will
    // see is exactly one walk launch on an empty table, no log -- what a plan can be built from.
    Dev<unsigned short> plan_rank;
    Dev<u64> plan_lo, plan_hi;
    u32 plan_n = 0;
    bool plan_valid = false, plan_stale = false, plan_src_ok = false;
    int plan_budget = 0;
    bool walk_no_plan = false;   // KMC_WALK_NO_PLAN=1 at kmc_create: no plan is built, no plan launch queued
    // The plan launch is armed for ONE finalize: the one numbered plan_seq, and only while that finalize would be the next
    // thing queued on this ctx (plan_req_seq == plan_seq; anything else that is queued first clears it).  No two plan launches
    // ever carry the same number: arming skips the numbers handed out before.
    u64 plan_seq = 0, plan_req_seq = 0;   // (plan_seq: the last plan launch's number until its status has been booked)
    u64 plan_seq_max = 0;                 // the largest number a plan launch has carried
    Pin<u64> h_plan;             // pinned: the request and status words (KMC_PLAN_W_*): words of their own, nothing copies over them
    u64* d_plan = nullptr;       // h_plan as the device sees it (an alias, not an owner)
    // KMC_ALGO_SORT: scratch for one sub-batch and the sorted (key,count) runs produced so far
    DevBuf s_lo[2], s_hi[2];
    // the walk kernel's log of steps that fell off its LDS memo (kmc_walk.hip.h SkLog, kmc_sklog.hip.h): per-workgroup spans,
    // their fill counts, the 1024 hash bins the records are partitioned into, the bins' cursors
    DevBuf lg_rec, lg_count, lg_bins, lg_cursor;
    bool sklog_on = false;   // this data source overflows the LDS memo (a poll saw (k+16)-mers in the second-level table): log from now on
    DevBuf a_hist, a_rand, a_ror;   // level-0 histogram rows / AND / OR words of the accumulated key ranges (kmc_extract.hip.h)
    // KMC_ALGO_SORT accumulates: a batch only EXTRACTS its keys behind those of the batches before it (s_lo[0] /
    // s_hi[0]); they are sorted into ONE run when somebody needs the result (kmc_finalize, a reduce) or when 2^31
    // positions have come together.  (Sorting batch by batch left one run per batch -- 16 for a 1 GB file read in
    // 64 MB chunks -- and kmc_finalize then merged them by sorting everything once more: 0.9 s for 760 M 63-mers.)
    u64 acc_n = 0;           // key positions accumulated and not yet sorted
    u64 acc_hint = 0;        // positions the caller expects in all (kmc_count_file: the file size); sizes the first allocation
    DevBuf lr_rank;  // LR mode: rank of every position's 27-mer among the batch's distinct 27-mers
    // hand-written MSD radix sort (kmc_msd.hip.h): per-range histograms, segment lists, terminals
    DevBuf m_hist, m_stot, m_bsum, m_rmin, m_rmax, m_seg[2], m_first, m_cbase, m_skip, m_term, m_ord, m_bitmap, m_rank, m_nd, m_base, m_ctl, m_clist, m_w[2];
    Pin<MsdCtl> h_ctl;        // pinned mirror of the sort's device counters
    struct Run { Dev<u64> hi, lo, cnt; u64 n = 0, cap = 0; u64 total = 0; bool total_known = false; };
    std::vector<Run> runs;       // live runs
    std::vector<Run> run_pool;   // buffers of dropped runs, reused (multi-GB hipMalloc/hipFree per batch is slow)
    Run view_run;                // the merged, sorted view built by the last kmc_finalize (table entries + runs)
    const u64 *v_hi = nullptr, *v_lo = nullptr, *v_cnt = nullptr;  // the sorted view of the last finalize: aliases of o, of runs[0] or of view_run, not owners
    bool msd_dup_heavy = false;  // the last large unweighted sort collapsed its keys more than fourfold (leaf size of two-word sorts)
    bool prefer_sort = false;  // AUTO: the data source proved high-cardinality  // per-workgroup memo slots, kept across launches (kmc_walk.hip.h)

    // hipEvent pairs bracketing every count-kernel launch, batch by batch: a batch's events are read once they have
    // completed (harvest_timing), possibly several batches later -- a caller that never synchronises this ctx (the
    // multi-GPU step: count, pack, reset) still gets every batch's kernel time into kernel_ms_lifetime
    struct TimedBatch { std::vector<hipEvent_t> ev; int algo = 0; u64 n_bases = 0; u32 count_launches = 0; };
    std::deque<TimedBatch> tb;                // batches whose events have not been read yet (front = oldest)
    // KMC_ALGO_AUTO chooses by MEASURED cost: kernel milliseconds per base of this ctx's recent walk-path batches (walk
    // kernel + (k+16)-mer unfold + the table merge at finalize) and sort-path batches (< 0: not measured yet)
    double walk_ms_per_base = -1.0, sort_ms_per_base = -1.0;
    bool sort_by_cost = false;   // AUTO: the last comparison of the two rates said "sort" (prefer_sort: structural -- the source overflowed everything)
    std::vector<hipEvent_t> ev_free;          // events to reuse
    kmc_stats st{};
    int fin_parity = 0;    // which OUT/SUM counter pair the next kmc_finalize uses
    u64 fin_hint = 0;      // table entries at the last kmc_finalize (sizes the next speculative small-table finalize)
    // The rank sort of kmc_small_finalize_kernel is quadratic: 16 us for 1 k keys, 0.24 ms for 24 k, 0.8 ms for 68 k (measured).  The
    // weighted radix sort that larger tables take costs 0.25-0.3 ms at that size (a dozen small launches, two polls): tables
    // that were larger than this at the last finalize go there directly.  (KMC_FIN_SMALL_MAX overrides: the parity test of
    // the kernel's size boundaries runs it up to its limit, KMC_FIN_KERNEL_MAX.)
    u64 fin_small_max = 40000;
    // Sub-batch sizes of the sort path and of LR mode (run_sort_path, count_lr): the defaults are what the u32 indices of
    // the run kernels and 32 GiB of keys in flight allow.  KMC_SORT_SUB_CHUNKS / KMC_LR_SUB_STARTS turn them down (never
    // up) so that tests/test_sub_batches_gpu.py crosses sub-batch edges on inputs the CPU oracle can count.
    u64 sort_sub_chunks = 1ull << 21;   // chunks per sort: a multiple of KMC_MSD_RANGE / KMC_CHUNK in [64, 2^21]
    u64 lr_sub_starts = 1ull << 25;     // window starts per LR pass: a multiple of KMC_LRX_POS in [256, 2^25]
    bool view_unsynced = false;   // the last small-table finalize was waited for through the mirror, not the stream (poll_fin)
    bool batch_pending = false;  // a COUNT kernel (unknown number of new keys) is queued since the last poll
    u64 unpolled_adds = 0;       // upper bound of keys added by merge kernels since the last poll
    bool walk_overflowed = false;  // the last WALK/STREAM launches counted >5% of their k-mers with global atomics
                                   // (memo / LDS table overflow = high-cardinality input)
    u64 direct_seen = 0, kmers_seen = 0;
    bool pending = false;  // a batch has been queued since the last counter poll
    double rho_last = 0.0; // same, over the most recent sub-batch
    double rho_hist = -1.0; // new keys per k-mer of the previous batch as a whole (< 0: no history); survives kmc_reset
    bool b_open = false; double b_rho_max = 0.0; u64 b_occ0 = 0, b_kmers = 0;  // the batch whose last launch is still unobserved
    double rho_max = 0.0;  // largest observed (new distinct) / (k-mers) over a sub-batch
    int n_cu = 256;
    // A launch sized by a prediction (more k-mers than the table and spill area absorb for certain) is
    // "risky": the table is saved first, and if the spill area overflows the table is put back and the
    // rest of the batch is counted by the sort path, which needs no table (recover_overflow).
    struct Risky {
        bool armed = false;
        int mode = 0;                 // 1: entries listed in occ_list; 2: whole table copied
        bool empty = false;           // mode 1 and the table held nothing: there is nothing to save (no kernel)
        const uint8_t* d_bases = nullptr; const u64* d_offsets = nullptr; u64 n_reads = 0, n_bases = 0;
        u64 base_from = 0;            // first base position the risky launch covers ...
        const u64* d_from = nullptr;  // ... or where to read it on the device (end of the last piece walked before)
        u64 ctr[KMC_CTR_N] = {0};     // the device counters before the launch
    } risky;
    DevBuf snap_hi, snap_lo, snap_cnt, snap_n, snap_occ;
    // second-level memo of the walk kernel: (k+16)-mer table (kmc_walk.hip.h); three key words for k >= 48
    Table sk;
    u64* d_sk_counters = nullptr;   // the second half of d_counters (an alias, not an owner)
    u64* h_sk_counters = nullptr;   // the second half of h_counters, valid after a poll (an alias, not an owner)
    Dev<u64> sk_spill_hi, sk_spill_lo, sk_spill_cnt, sk_spill_mid;
    u64 sk_spill_cap = 0;
    Dev<u64> sk_occ;                // list of its claimed slots (what the unfold kernel walks)
    bool recovered = false;  // the last poll found an overflow and recovered: the batch in flight is complete
    bool sk_dirty = false;   // walk launches since the last unfold of the (k+16)-mer table
    bool sk_fixed = false;   // its size was set by KMC_SK_SLOTS (tests): never re-allocated
    bool sk_grow = false;    // a poll found it more than half full: re-allocate larger when it is next empty
    KeyBufs rx;  // receive buffers of the one-process multi-GPU reduce (a peer's sorted table)
    // kmc_filter_device's result (its own buffers: a filter leaves the view and a partition the caller holds alone);
    // kmc_histogram's device histogram + max
    KeyBufs f;
    DevBuf h_hist;
    // scratch of a compaction (compact_plan): kept entries per tile, their scan, its block sums, the control words.  The
    // filter and the set operations share it: both are done with it when their call returns.
    DevBuf c_tile, c_tpos, c_bsum, c_ctl;
    // kmc_query / kmc_profile (kmc_query.hip.h): the prefix index of the view numbered q_gen (view_gen counts the views this
    // ctx has produced: every place that publishes one bumps it, so an index can never outlive its view), staging of the
    // host forms: query keys and counts, a batch's bases and offsets, its window counts and read statistics
    u64 view_gen = 0, q_gen = ~0ull;
    DevBuf q_idx, q_khi, q_klo, q_cnt, q_bases, q_offs, q_win, q_stats;
    // kmc_compare / kmc_setop_device (kmc_setops.hip.h), on the ctx given as `a`: the result, the merge-path partition of the
    // two views (first A / B entry of every tile)
    KeyBufs so;
    DevBuf so_pa, so_pb;
    // kmc_graph / kmc_graph_device (kmc_graph.hip.h): one 16-bit word per key of the view, the eight summary words
    DevBuf g_adj, g_ctl;
    // kmc_unitigs / kmc_unitigs_device (kmc_unitig.hip.h): the result (bases, offsets, abundances, flags), and the work
    // arrays over the 2n side states -- links, joins, two (pointer, distance) pairs of the ranking -- the cycle marks per
    // key, the summary words and round counts.  u_key / u_words: the view and the range the result arrays were computed
    // for (ResultKey) and their summary, so that kmc_unitigs' sizing call and the copy call that follows it compute once
    DevBuf u_bases, u_offs, u_abund, u_flags;
    ResultKey u_key;
    u64 u_words[8] = {};
    DevBuf u_link, u_join, u_ptr[2], u_dist[2], u_circ, u_ctl;
    // kmc_unitig_links / kmc_unitig_links_device (kmc_links.hip.h) read what unitig_run left besides its result: adj, the
    // final ranking u_ptr[u_cur] / u_dist[u_cur], the unitig ids in u_join.  u_live is a different fact from u_key: not
    // "the result arrays hold this result" but "the WORK arrays are still this result's": unitig_run sets it when it is
    // through, anything that rewrites adj (graph_run) clears it, and the result itself stays good.
    // The result (offsets per end, targets) with l_key / l_words as above, the work arrays per end
    // (counts, their scan), the resolved targets per view row, the control words.
    int u_cur = 0;
    bool u_live = false;
    DevBuf l_offs, l_to, l_cnt, l_pos, l_tgt, l_ctl;
    ResultKey l_key;
    u64 l_words[8] = {};
    // kmc_unitig_map / kmc_unitig_map_device (kmc_map.hip.h) read the same work arrays.  m_idx is the row index built from
    // them -- per view row the unitig, the key position and the strand -- and m_idx_live says it is still theirs: map_run
    // sets it, graph_run (which every unitig_run goes through) clears it.  The result of the last call: place words, per-read
    // rows, segment offsets and records, support per unitig; between the passes the read-start and valid-window bits of
    // the batch and the tails' positions.
    DevBuf m_idx, m_place, m_stats, m_soffs, m_segs, m_support, m_sbits, m_vbits, m_tail;
    bool m_idx_live = false;
    // kmc_correct / kmc_correct_device (kmc_correct.hip.h) read the view and the query index alone.  The result of the last
    // call: the corrected copy of the batch, per-read rows, candidate offsets and records; between the passes the
    // read-start, valid-window and weak-window bits of the batch and, per candidate, its batch position and read.
    DevBuf cr_out, cr_stats, cr_coffs, cr_cands, cr_where, cr_sbits, cr_vbits, cr_wbits;
    // kmc_trim / kmc_trim_device (kmc_trim.hip.h) read the view and the query index alone.  The result of the last call: the
    // emitted spans as a batch (bases and offsets in two buffers each, written in turn: tr_cur is the pair of the last call,
    // so a caller may hand that result back in), the source read of each, per-read rows and verdicts.  Between the passes:
    // the bit arrays of the mark pass (its own, a correct result stays as it is), six words of runs per read, the list of
    // the reads a wave or a workgroup reduces, the emitted flags and span lengths with their scans, each span's batch position.
    DevBuf tr_out[2], tr_ooffs[2], tr_origin, tr_stats, tr_verdict;
    DevBuf tr_sbits, tr_vbits, tr_wbits, tr_runs, tr_list, tr_emit, tr_elen, tr_epos, tr_lpos, tr_src;
    int tr_cur = 0;
    // kmc_normalize / kmc_normalize_device (kmc_normalize.hip.h) read the view and the query index alone.  The result of the
    // last call: the emitted reads as a batch, the source read of each, per-read rows and verdicts (one buffer each: the call
    // refuses its own result as input).  Between the passes: the profile pass's window counts and per-read rows (its own, no
    // call hands them out), a depth per read, the list of the reads a workgroup selects, the emitted flags and lengths with
    // their scans, each emitted read's batch position.
    DevBuf nm_out, nm_ooffs, nm_origin, nm_stats, nm_verdict;
    DevBuf nm_win, nm_pstats, nm_depth, nm_list, nm_emit, nm_elen, nm_epos, nm_lpos, nm_src;
    // kmc_unitig_clean* and kmc_unitig_simplify* (kmc_clean.hip.h) read the unitigs, the links and what the links pass
    // reads.  Their result: the verdict per unitig and the kept table, with cl_key plus its three limits cl_tip / cl_isl /
    // cl_bub (0 for a clean call) and cl_words as above (nothing but the clean pass writes them; a clean call hands out the
    // first 8), cl_kept keys; the class byte per view row between its two passes; the totals per workgroup of a mark
    // pass that pops bubbles.
    KeyBufs cl;
    DevBuf cl_verdict, cl_row, cl_part;
    ResultKey cl_key;
    u64 cl_tip = 0, cl_isl = 0, cl_bub = 0, cl_kept = 0, cl_words[12] = {};
    // kmc_unitig_components* (kmc_components.hip.h) read the unitigs and the links.  Their result, in buffers of their own
    // (a clean / simplify result stays as it is): the component per unitig, four words per component, the verdict per
    // unitig and the kept table, with cc_key plus its limit cc_limit and cc_words as above, cc_comps components and
    // cc_kept keys.  Whatever drops l_key drops cc_key.  Work arrays: the parents of the label rounds, the root flags and
    // their scan, the totals per workgroup of the summary pass, the control words and round counters.
    KeyBufs cc;
    DevBuf cc_comp, cc_stats, cc_verdict, cc_parent, cc_flag, cc_rank, cc_part, cc_ctl;
    ResultKey cc_key;
    u64 cc_limit = 0, cc_kept = 0, cc_comps = 0, cc_words[8] = {};
    // kmc_unitig_bubbles* (kmc_bubbles.hip.h) read the unitigs and the links.  Their result, in a buffer of its own (a clean /
    // simplify / components result stays as it is): eight words per called unitig, with bb_key plus its limit bb_limit and
    // bb_words as above, bb_records records.  Whatever drops l_key drops bb_key.  Work arrays: the called flag per unitig,
    // its scan, major(u), the control words.
    DevBuf bb_rec, bb_flag, bb_pos, bb_major, bb_ctl;
    ResultKey bb_key;
    u64 bb_limit = 0, bb_records = 0, bb_words[8] = {};
    // kmc_unitig_transits* (kmc_transits.hip.h) read the links and the segments of a map call.  Their result, in buffers of
    // their own (a map, correct, trim, normalize or profile call leaves them alone, and KMC_TRANSIT_ACCUMULATE adds onto
    // them): support per link record, the slot offsets per unitig, the slots, the verdict per unitig, with tx_key and
    // tx_words as above and tx_slots slots.  Whatever drops l_key drops tx_key.  Work arrays: the slots per unitig and
    // their scan, the first-segment byte per segment of the batch, the control words.
    DevBuf tx_sup, tx_offs, tx_count, tx_verdict, tx_cnt, tx_pos, tx_first, tx_ctl;
    ResultKey tx_key;
    u64 tx_slots = 0, tx_words[8] = {};
    // kmc_unitig_contigs* (kmc_contigs.hip.h) read the unitig arrays, the links and the transit counts.  Their result, in
    // buffers of their own: bases, offsets, path offsets, path, abundances, flags, with ct_key plus its two parameters
    // ct_reads / ct_support and ct_words as above.  Whatever drops l_key or tx_key drops ct_key, and so does every transits
    // call (the counts changed).  Work arrays: copies and sigma per unitig, node_offsets, the unitig of a node; over the
    // 2 * n_nodes node ends what u_link .. u_circ are over the side states (the unitigs' own stay as they are: a links or
    // map call may still read them); per path slot its contig, key count, their scan, start base and source base; the
    // control words and round counts.
    DevBuf ct_bases, ct_offs, ct_poffs, ct_path, ct_abund, ct_flags;
    DevBuf ct_copies, ct_sigma, ct_pos, ct_owner, ct_link, ct_join, ct_ptr[2], ct_dist[2], ct_circ, ct_cid, ct_keys, ct_g, ct_start, ct_src, ct_ctl;
    ResultKey ct_key;
    u64 ct_reads = 0, ct_support = 0, ct_words[8] = {};
    // kmc_unitig_pairs* (kmc_pairs.hip.h) read the unitig offsets and the segments of a map call.  Their result, in buffers
    // of their own (a map, transits or contigs call leaves them alone, and KMC_PAIR_ACCUMULATE adds onto them): per pair of
    // the last batch the class, the two ends and the value; the record set pr_cur of two -- sort key, ends, count, sum, min,
    // max per record, the other set is where the next ACCUMULATE call builds its own -- and the insert histogram, with pr_key
    // plus its parameter pr_bins and pr_words as above and pr_records records.  Whatever recomputes the unitigs drops pr_key;
    // the links do not matter to it.  Work arrays: the anchor row per read, the sort keys and weights with the sort's
    // scratch copies, the control words.
    DevBuf pr_class, pr_ends, pr_value, pr_hist;
    DevBuf pr_rkey[2], pr_rends[2], pr_rcount[2], pr_rsum[2], pr_rmin[2], pr_rmax[2];
    DevBuf pr_anchor, pr_sk[2], pr_sw[2], pr_ctl;
    ResultKey pr_key;
    int pr_cur = 0;
    u64 pr_bins = 0, pr_records = 0, pr_words[8] = {};
};

#pragma GCC visibility push(hidden)   // what follows is shared between the translation units, never exported

extern thread_local char g_create_err[512];   // kmc_last_error(nullptr): why kmc_create failed (kmc_api.hip)

inline int fail(kmc_ctx* c, int code, const char* fmt, ...) {
    char buf[512] = {0};
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    memcpy(c ? c->err : g_create_err, buf, sizeof(buf));
    return code;
}

#define HIPCHK(c, call)                                                                       \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess)                                                                \
            return fail((c), e__ == hipErrorOutOfMemory ? KMC_ERR_NOMEM : KMC_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

inline int ensure(kmc_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return KMC_OK;
    HIPCHK(c, b.alloc(bytes + bytes / 8 + 256));
    return KMC_OK;
}

// room for n entries (one at least), the high words for two-word keys only
inline int ensure_keys(kmc_ctx* c, KeyBufs& k, u64 n) {
    const size_t nb = (size_t)std::max<u64>(n, 1) * sizeof(u64);
    int rc = ensure(c, k.lo, nb);
    if (!rc) rc = ensure(c, k.cnt, nb);
    if (!rc && c->KW == 2) rc = ensure(c, k.hi, nb);
    return rc;
}

// the device pointers as the ABI returns them (each optional; no high words for one-word keys)
inline void publish_keys(const kmc_ctx* c, const KeyBufs& k, const void** d_key_hi, const void** d_key_lo, const void** d_count) {
    if (d_key_hi) *d_key_hi = c->KW == 2 ? k.hi.p : nullptr;
    if (d_key_lo) *d_key_lo = k.lo.p;
    if (d_count) *d_count = k.cnt.p;
}

inline int grid_for(const kmc_ctx* c, u64 n, int threads) {
    return (int)std::max<u64>(1, std::min<u64>((n + threads - 1) / threads, (u64)c->n_cu * 8));
}

// What the calls that read the view do first: a finalize queued by kmc_finalize_async counts as one (kmc_api.hip)
int resolve_view(kmc_ctx* c);

// The second thing the view layer calls of the counting side (kmc_api.hip): the MSD radix sort with run-length on n
// one-word keys of key_bits < 64 bits in lo[0], their weights in w[0]; lo[1] / w[1] are scratch of the same size and
// all four are overwritten.  Keys with a bit at or above key_bits are filler and dropped.  out gets the sorted distinct
// keys (out->lo), the sums of their weights (out->cnt) and out->n / out->total; give it back with recycle_run when the
// stream is through with it.  It works in the sort's scratch (m_*, h_ctl) and the run pool alone: the view, the live runs
// and the keys extracted and not yet sorted stay as they are, and so does what the sort path has learned about its keys.
int sort_keys_to_run(kmc_ctx* c, u64* const lo[2], u64* const w[2], u64 n, unsigned key_bits, kmc_ctx::Run* out);
void recycle_run(kmc_ctx* c, kmc_ctx::Run* r);

// no C++ exception leaves the library (kmc.h: "no exception or abort crosses the ABI")
template <typename F>
int guarded(kmc_ctx* c, F&& f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(c, KMC_ERR_NOMEM, "out of host memory");
    } catch (const std::exception& e) {
        return fail(c, KMC_ERR_HIP, "internal error: %s", e.what());
    } catch (...) {
        return fail(c, KMC_ERR_HIP, "internal error (unknown C++ exception)");
    }
}

#pragma GCC visibility pop
