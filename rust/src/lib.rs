//! Rust binding of `include/kmc.h` (libkmc.so).  NOT COMPILED in the build environment of this
//! repository (no rustc there); a CPU test parses this file and checks every declaration against the
//! header (tests/test_abi_host.py::test_rust_binding_matches_the_header).
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

pub const KMC_MODE_CONTIG: i32 = 0;
pub const KMC_MODE_LR: i32 = 1;
pub const KMC_ALGO_AUTO: i32 = 0;
pub const KMC_ALGO_STREAM: i32 = 1;
pub const KMC_ALGO_WALK: i32 = 2;
pub const KMC_ALGO_SORT: i32 = 3;
pub const KMC_FORGET_MEMO: c_int = 1;
pub const KMC_FORGET_HISTORY: c_int = 2;
/// words per read of `kmc_profile`'s read_stats
pub const KMC_PROFILE_WORDS: usize = 5;
pub const KMC_COMPARE_WORDS: usize = 8;
pub const KMC_SETOP_INTERSECT: i32 = 0;
pub const KMC_SETOP_UNION: i32 = 1;
pub const KMC_SETOP_SUBTRACT: i32 = 2;
pub const KMC_COUNT_LEFT: i32 = 0;
pub const KMC_COUNT_RIGHT: i32 = 1;
pub const KMC_COUNT_MIN: i32 = 2;
pub const KMC_COUNT_MAX: i32 = 3;
pub const KMC_COUNT_SUM: i32 = 4;
pub const KMC_COUNT_DIFF: i32 = 5;
/// summary words of `kmc_graph`
pub const KMC_GRAPH_WORDS: usize = 8;
/// summary words of `kmc_unitigs`
pub const KMC_UNITIG_WORDS: usize = 8;
/// bit 0 of a unitig's flags byte
pub const KMC_UNITIG_CIRCULAR: u8 = 1;
/// summary words of `kmc_unitig_links`
pub const KMC_LINK_WORDS: usize = 8;
/// summary words of `kmc_unitig_map`, words per read of its `read_stats`, the low half of the place word of a window
/// that is not placed
pub const KMC_MAP_WORDS: usize = 8;
pub const KMC_MAP_READ_WORDS: usize = 4;
pub const KMC_MAP_NONE: u32 = 0xFFFF_FFFF;
/// summary words of `kmc_unitig_transits`, a unitig's verdict, the flag that adds onto the held result
pub const KMC_TRANSIT_WORDS: usize = 8;
pub const KMC_TRANSIT_PLAIN: u8 = 0;
pub const KMC_TRANSIT_UNSPANNED: u8 = 1;
pub const KMC_TRANSIT_RESOLVED: u8 = 2;
pub const KMC_TRANSIT_AMBIGUOUS: u8 = 3;
pub const KMC_TRANSIT_ACCUMULATE: u32 = 1;
/// summary words of `kmc_unitig_pairs`, a pair's class byte, the flag that adds onto the held result
pub const KMC_PAIR_WORDS: usize = 8;
pub const KMC_PAIR_UNPLACED: u8 = 0;
pub const KMC_PAIR_SPAN: u8 = 1;
pub const KMC_PAIR_PROPER: u8 = 2;
pub const KMC_PAIR_EVERTED: u8 = 3;
pub const KMC_PAIR_SAME_STRAND: u8 = 4;
pub const KMC_PAIR_ACCUMULATE: u32 = 1;
/// summary words of `kmc_unitig_contigs`
pub const KMC_CONTIG_WORDS: usize = 8;
/// summary words of `kmc_correct`, words per read of its `read_stats`, the kinds of a candidate
pub const KMC_CORRECT_WORDS: usize = 8;
pub const KMC_CORRECT_READ_WORDS: usize = 4;
pub const KMC_CORRECT_INTERIOR: u32 = 0;
pub const KMC_CORRECT_HEAD: u32 = 1;
pub const KMC_CORRECT_TAIL: u32 = 2;
/// summary words of `kmc_trim`, words per read of its `read_stats`, its modes, flag bits and verdict bits
pub const KMC_TRIM_WORDS: usize = 8;
pub const KMC_TRIM_READ_WORDS: usize = 4;
pub const KMC_TRIM_NONE: c_int = 0;
pub const KMC_TRIM_ENDS: c_int = 1;
pub const KMC_TRIM_LONGEST: c_int = 2;
pub const KMC_TRIM_INVERT: u32 = 1;
pub const KMC_TRIM_PAIR_BOTH: u32 = 2;
pub const KMC_TRIM_PAIR_EITHER: u32 = 4;
pub const KMC_TRIM_PASS: u8 = 1;
pub const KMC_TRIM_EMITTED: u8 = 2;
/// summary words of `kmc_normalize`, words per read of its `read_stats`, its flag bits and verdict bits
pub const KMC_NORMALIZE_WORDS: usize = 8;
pub const KMC_NORMALIZE_READ_WORDS: usize = 4;
pub const KMC_NORM_PAIRED: u32 = 1;
pub const KMC_NORM_INVERT: u32 = 2;
pub const KMC_NORM_KEEP: u8 = 1;
pub const KMC_NORM_EMITTED: u8 = 2;
pub const KMC_NORM_LOW: u8 = 4;
pub const KMC_NORM_DEEP: u8 = 8;
/// summary words of `kmc_unitig_clean`
pub const KMC_CLEAN_WORDS: usize = 8;
/// a unitig's verdict byte
pub const KMC_CLEAN_KEEP: u8 = 0;
pub const KMC_CLEAN_TIP: u8 = 1;
pub const KMC_CLEAN_ISLAND: u8 = 2;
/// the fourth verdict, of `kmc_unitig_simplify`
pub const KMC_CLEAN_BUBBLE: u8 = 3;
/// summary words of `kmc_unitig_simplify`
pub const KMC_SIMPLIFY_WORDS: usize = 12;
/// summary words of `kmc_unitig_components`, words per component of its `comp_stats`, the verdict of a small component's unitigs
pub const KMC_COMPONENT_WORDS: usize = 8;
pub const KMC_COMPONENT_STAT_WORDS: usize = 4;
pub const KMC_CLEAN_COMPONENT: u8 = 4;
/// summary words of `kmc_unitig_bubbles`, words per record, a record's kind (bits 0-1 of word 6) and its flag bit
pub const KMC_BUBBLE_WORDS: usize = 8;
pub const KMC_BUBBLE_RECORD_WORDS: usize = 8;
pub const KMC_BUBBLE_SUBST: u32 = 0;
pub const KMC_BUBBLE_INDEL: u32 = 1;
pub const KMC_BUBBLE_COMPLEX: u32 = 2;
pub const KMC_BUBBLE_REVERSED: u32 = 4;

// The structs and the extern block below are checked against include/kmc.h by
// tests/test_abi_host.py::test_rust_binding_matches_the_header (names, arity, argument types, field
// order and types), because no Rust toolchain exists in the build environment to do it.
#[repr(C)]
pub struct KmcConfig {
    pub struct_size: u32,
    pub k: i32,
    pub mode: i32,
    pub canonical: i32,
    pub device: i32,
    pub algo: i32,
    pub capacity_hint: u64,
    pub stream: *mut c_void,
}

#[repr(C)]
pub struct KmcStats {
    pub n_reads: u64,
    pub n_bases: u64,
    pub n_kmers: u64,
    pub n_distinct: u64,
    pub table_capacity: u64,
    pub n_spilled: u64,
    pub n_batches: u64,
    pub kernel_ms_last: f64,
    pub kernel_ms_total: f64,
    pub algo_last: i32,
    pub launches_last: i32,
    pub n_slabs_skipped: u64,
    pub n_direct: u64,
    pub kernel_ms_lifetime: f64,
    pub launches_lifetime: u64,
    pub n_async_ok: u64,
    pub n_async_slabs_skipped: u64,
    pub n_planner_stale: u64,
    pub walk_uniform_launches: u64,
    pub walk_plan_finalizes: u64,
    pub walk_plan_builds: u64,
}

#[repr(C)]
pub struct KmcReads {
    pub bases: *mut u8,
    pub offsets: *mut u64,
    pub n_reads: u64,
    pub n_bases: u64,
    pub max_read_len: u64,
}

#[repr(C)]
pub struct KmcSynth {
    pub seed: u64,
    pub pool: u32,
    pub line_len: u32,
    pub lines_per_record: u32,
    pub reserved: u32,
}

#[repr(C)]
pub struct KmcCtx {
    _private: [u8; 0],
}

#[repr(C)]
pub struct KmcFastaStream {
    _private: [u8; 0],
}

extern "C" {
    pub fn kmc_version() -> *const c_char;
    pub fn kmc_status_string(status: c_int) -> *const c_char;
    pub fn kmc_create(out: *mut *mut KmcCtx, cfg: *const KmcConfig) -> c_int;
    pub fn kmc_destroy(ctx: *mut KmcCtx);
    pub fn kmc_last_error(ctx: *const KmcCtx) -> *const c_char;
    pub fn kmc_reset(ctx: *mut KmcCtx) -> c_int;
    pub fn kmc_add_batch(ctx: *mut KmcCtx, bases: *const u8, offsets: *const u64, n_reads: u64) -> c_int;
    pub fn kmc_add_batch_device(ctx: *mut KmcCtx, d_bases: *const c_void, d_offsets: *const c_void, n_reads: u64, n_bases: u64, max_read_len: u64) -> c_int;
    pub fn kmc_merge_pairs_device(ctx: *mut KmcCtx, d_key_hi: *const c_void, d_key_lo: *const c_void, d_count: *const c_void, n_pairs: u64) -> c_int;
    pub fn kmc_finalize(ctx: *mut KmcCtx, n_distinct: *mut u64, n_total: *mut u64) -> c_int;
    pub fn kmc_export(ctx: *mut KmcCtx, key_hi: *mut u64, key_lo: *mut u64, count: *mut u64, cap: u64) -> c_int;
    pub fn kmc_export_device(ctx: *mut KmcCtx, d_key_hi: *mut *const c_void, d_key_lo: *mut *const c_void, d_count: *mut *const c_void, n_distinct: *mut u64) -> c_int;
    pub fn kmc_partition_device(ctx: *mut KmcCtx, n_parts: u32, part_begin: *mut u64, d_key_hi: *mut *const c_void,
                                d_key_lo: *mut *const c_void, d_count: *mut *const c_void) -> c_int;
    pub fn kmc_owner_of(key_hi: u64, key_lo: u64, n_parts: u32) -> u32;
    pub fn kmc_histogram(ctx: *mut KmcCtx, min_count: u64, max_count: u64, n_bins: u32, hist: *mut u64, max_seen: *mut u64) -> c_int;
    pub fn kmc_filter_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, d_key_hi: *mut *const c_void, d_key_lo: *mut *const c_void,
                             d_count: *mut *const c_void, n_kept: *mut u64, kept_total: *mut u64) -> c_int;
    pub fn kmc_export_filtered(ctx: *mut KmcCtx, min_count: u64, max_count: u64, key_hi: *mut u64, key_lo: *mut u64, count: *mut u64,
                               cap: u64, n_kept: *mut u64) -> c_int;
    // asking the table: key lookups and per-read profiles of the sorted view
    pub fn kmc_encode_key(kmer: *const c_char, klen: c_int, canonical: c_int, key_hi: *mut u64, key_lo: *mut u64) -> c_int;
    pub fn kmc_query(ctx: *mut KmcCtx, key_hi: *const u64, key_lo: *const u64, n_keys: u64, count: *mut u64) -> c_int;
    pub fn kmc_query_device(ctx: *mut KmcCtx, d_key_hi: *const c_void, d_key_lo: *const c_void, n_keys: u64, d_count: *mut c_void) -> c_int;
    pub fn kmc_profile(ctx: *mut KmcCtx, bases: *const u8, offsets: *const u64, n_reads: u64, min_count: u64, window_count: *mut u32,
                       read_stats: *mut u64) -> c_int;
    pub fn kmc_profile_device(ctx: *mut KmcCtx, d_bases: *const c_void, d_offsets: *const c_void, n_reads: u64, n_bases: u64,
                              min_count: u64, d_window_count: *mut c_void, d_read_stats: *mut c_void) -> c_int;
    // two tables: summary and set operations over the sorted views of two contexts
    pub fn kmc_compare(a: *mut KmcCtx, b: *mut KmcCtx, min_a: u64, max_a: u64, min_b: u64, max_b: u64, summary: *mut u64) -> c_int;
    pub fn kmc_setop_device(a: *mut KmcCtx, b: *mut KmcCtx, op: c_int, count_mode: c_int, min_a: u64, max_a: u64, min_b: u64, max_b: u64,
                            d_key_hi: *mut *const c_void, d_key_lo: *mut *const c_void, d_count: *mut *const c_void, n_out: *mut u64,
                            total_out: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_export_setop(a: *mut KmcCtx, b: *mut KmcCtx, op: c_int, count_mode: c_int, min_a: u64, max_a: u64, min_b: u64, max_b: u64,
                            key_hi: *mut u64, key_lo: *mut u64, count: *mut u64, cap: u64, n_out: *mut u64) -> c_int;
    // the table as a de Bruijn graph: neighbour masks, unitig ends, summary (adj: uint16_t per key of the view)
    pub fn kmc_graph_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, d_adj: *mut *const c_void, n_keys: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_graph(ctx: *mut KmcCtx, min_count: u64, max_count: u64, adj: *mut c_void, cap: u64, n_keys: *mut u64, summary: *mut u64) -> c_int;
    // the unitigs of that graph: bases + offsets, abundances, flags, summary
    pub fn kmc_unitigs_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, d_bases: *mut *const c_void, d_offsets: *mut *const c_void, d_abund: *mut *const c_void, d_flags: *mut *const c_void, n_unitigs: *mut u64, n_bases: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitigs(ctx: *mut KmcCtx, min_count: u64, max_count: u64, bases: *mut u8, cap_bases: u64, offsets: *mut u64, abund: *mut u64, flags: *mut u8, cap_unitigs: u64, n_unitigs: *mut u64, n_bases: *mut u64, summary: *mut u64) -> c_int;
    // the links between those unitigs: offsets per unitig end, target ends, summary
    pub fn kmc_unitig_links_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, d_link_offsets: *mut *const c_void, d_link_to: *mut *const c_void, n_unitigs: *mut u64, n_links: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_links(ctx: *mut KmcCtx, min_count: u64, max_count: u64, link_offsets: *mut u64, cap_ends: u64, link_to: *mut u32, cap_links: u64, n_unitigs: *mut u64, n_links: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_map_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, d_bases: *const c_void, d_offsets: *const c_void, n_reads: u64, n_bases: u64, d_place: *mut *const c_void, d_read_stats: *mut *const c_void, d_seg_offsets: *mut *const c_void, d_segs: *mut *const c_void, d_support: *mut *const c_void, n_segs: *mut u64, n_unitigs: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_map(ctx: *mut KmcCtx, min_count: u64, max_count: u64, bases: *const u8, offsets: *const u64, n_reads: u64, place: *mut u64, read_stats: *mut u32, seg_offsets: *mut u64, segs: *mut u32, cap_segs: u64, support: *mut u64, cap_unitigs: u64, n_segs: *mut u64, n_unitigs: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_transits_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, min_reads: u64, flags: u32, d_bases: *const c_void, d_offsets: *const c_void, n_reads: u64, n_bases: u64, d_link_support: *mut *const c_void, d_transit_offsets: *mut *const c_void, d_transit_count: *mut *const c_void, d_verdict: *mut *const c_void, n_unitigs: *mut u64, n_links: *mut u64, n_slots: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_transits(ctx: *mut KmcCtx, min_count: u64, max_count: u64, min_reads: u64, flags: u32, bases: *const u8, offsets: *const u64, n_reads: u64, link_support: *mut u64, cap_links: u64, transit_offsets: *mut u64, cap_unitigs: u64, transit_count: *mut u64, cap_slots: u64, verdict: *mut u8, n_unitigs: *mut u64, n_links: *mut u64, n_slots: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_pairs_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, n_bins: u64, flags: u32, d_bases: *const c_void, d_offsets: *const c_void, n_reads: u64, n_bases: u64, d_pair_class: *mut *const c_void, d_pair_ends: *mut *const c_void, d_pair_value: *mut *const c_void, d_rec_ends: *mut *const c_void, d_rec_count: *mut *const c_void, d_rec_sum: *mut *const c_void, d_rec_min: *mut *const c_void, d_rec_max: *mut *const c_void, d_insert_hist: *mut *const c_void, n_pairs: *mut u64, n_records: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_pairs(ctx: *mut KmcCtx, min_count: u64, max_count: u64, n_bins: u64, flags: u32, bases: *const u8, offsets: *const u64, n_reads: u64, pair_class: *mut u8, pair_ends: *mut u32, pair_value: *mut u64, cap_pairs: u64, rec_ends: *mut u32, rec_count: *mut u64, rec_sum: *mut u64, rec_min: *mut u64, rec_max: *mut u64, cap_records: u64, insert_hist: *mut u64, cap_bins: u64, n_pairs: *mut u64, n_records: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_contigs_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, min_reads: u64, min_support: u64, d_bases: *mut *const c_void, d_offsets: *mut *const c_void, d_path_offsets: *mut *const c_void, d_path: *mut *const c_void, d_abund: *mut *const c_void, d_flags: *mut *const c_void, n_contigs: *mut u64, n_nodes: *mut u64, n_bases: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_contigs(ctx: *mut KmcCtx, min_count: u64, max_count: u64, min_reads: u64, min_support: u64, bases: *mut u8, cap_bases: u64, offsets: *mut u64, path_offsets: *mut u64, abund: *mut u64, flags: *mut u8, cap_contigs: u64, path: *mut u32, cap_nodes: u64, n_contigs: *mut u64, n_nodes: *mut u64, n_bases: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_correct_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, d_bases: *const c_void, d_offsets: *const c_void, n_reads: u64, n_bases: u64, d_corrected: *mut *const c_void, d_read_stats: *mut *const c_void, d_cand_offsets: *mut *const c_void, d_cands: *mut *const c_void, n_cands: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_correct(ctx: *mut KmcCtx, min_count: u64, max_count: u64, bases: *const u8, offsets: *const u64, n_reads: u64, out_bases: *mut u8, read_stats: *mut u32, cand_offsets: *mut u64, cands: *mut u32, cap_cands: u64, n_cands: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_trim_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, mode: c_int, flags: u32, min_strong: u64, min_permille: u32, min_len: u64, d_bases: *const c_void, d_offsets: *const c_void, n_reads: u64, n_bases: u64, d_out_bases: *mut *const c_void, d_out_offsets: *mut *const c_void, d_origin: *mut *const c_void, d_read_stats: *mut *const c_void, d_verdict: *mut *const c_void, n_out: *mut u64, n_out_bases: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_trim(ctx: *mut KmcCtx, min_count: u64, max_count: u64, mode: c_int, flags: u32, min_strong: u64, min_permille: u32, min_len: u64, bases: *const u8, offsets: *const u64, n_reads: u64, out_bases: *mut u8, cap_bases: u64, out_offsets: *mut u64, origin: *mut u64, cap_reads: u64, read_stats: *mut u32, verdict: *mut u8, n_out: *mut u64, n_out_bases: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_normalize_device(ctx: *mut KmcCtx, permille: u32, target: u64, min_depth: u64, seed: u64, flags: u32, d_bases: *const c_void, d_offsets: *const c_void, n_reads: u64, n_bases: u64, d_out_bases: *mut *const c_void, d_out_offsets: *mut *const c_void, d_origin: *mut *const c_void, d_read_stats: *mut *const c_void, d_verdict: *mut *const c_void, n_out: *mut u64, n_out_bases: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_normalize(ctx: *mut KmcCtx, permille: u32, target: u64, min_depth: u64, seed: u64, flags: u32, bases: *const u8, offsets: *const u64, n_reads: u64, out_bases: *mut u8, cap_bases: u64, out_offsets: *mut u64, origin: *mut u64, cap_reads: u64, read_stats: *mut u32, verdict: *mut u8, n_out: *mut u64, n_out_bases: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_clean_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64, d_key_hi: *mut *const c_void, d_key_lo: *mut *const c_void, d_count: *mut *const c_void, d_verdict: *mut *const c_void, n_kept: *mut u64, n_unitigs: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_clean(ctx: *mut KmcCtx, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64, key_hi: *mut u64, key_lo: *mut u64, count: *mut u64, cap_keys: u64, verdict: *mut u8, cap_unitigs: u64, n_kept: *mut u64, n_unitigs: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_clean_into(src: *mut KmcCtx, dst: *mut KmcCtx, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_simplify_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64, max_bubble_keys: u64, d_key_hi: *mut *const c_void, d_key_lo: *mut *const c_void, d_count: *mut *const c_void, d_verdict: *mut *const c_void, n_kept: *mut u64, n_unitigs: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_simplify(ctx: *mut KmcCtx, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64, max_bubble_keys: u64, key_hi: *mut u64, key_lo: *mut u64, count: *mut u64, cap_keys: u64, verdict: *mut u8, cap_unitigs: u64, n_kept: *mut u64, n_unitigs: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_simplify_into(src: *mut KmcCtx, dst: *mut KmcCtx, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64, max_bubble_keys: u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_components_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, max_component_keys: u64, d_comp_of: *mut *const c_void, d_comp_stats: *mut *const c_void, d_verdict: *mut *const c_void, d_key_hi: *mut *const c_void, d_key_lo: *mut *const c_void, d_count: *mut *const c_void, n_comps: *mut u64, n_unitigs: *mut u64, n_kept: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_components(ctx: *mut KmcCtx, min_count: u64, max_count: u64, max_component_keys: u64, comp_of: *mut u32, verdict: *mut u8, cap_unitigs: u64, comp_stats: *mut u64, cap_comps: u64, key_hi: *mut u64, key_lo: *mut u64, count: *mut u64, cap_keys: u64, n_comps: *mut u64, n_unitigs: *mut u64, n_kept: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_components_into(src: *mut KmcCtx, dst: *mut KmcCtx, min_count: u64, max_count: u64, max_component_keys: u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_bubbles_device(ctx: *mut KmcCtx, min_count: u64, max_count: u64, max_bubble_keys: u64, d_records: *mut *const c_void, n_records: *mut u64, n_unitigs: *mut u64, summary: *mut u64) -> c_int;
    pub fn kmc_unitig_bubbles(ctx: *mut KmcCtx, min_count: u64, max_count: u64, max_bubble_keys: u64, records: *mut u32, cap_records: u64, n_records: *mut u64, n_unitigs: *mut u64, summary: *mut u64) -> c_int;
    // multi-GPU reduce (one process per GPU; the collective itself is the host program's, e.g. RCCL)
    pub fn kmc_slab_words(ctx: *const KmcCtx, slab_entries: u64) -> u64;
    pub fn kmc_pack_slab_device(ctx: *mut KmcCtx, d_slab: *mut c_void, slab_entries: u64) -> c_int;
    pub fn kmc_merge_slabs_device(ctx: *mut KmcCtx, d_slabs: *const c_void, n_slabs: u32, slab_entries: u64, my_part: u32, n_parts: u32) -> c_int;
    pub fn kmc_poll(ctx: *mut KmcCtx) -> c_int;
    pub fn kmc_sync(ctx: *mut KmcCtx) -> c_int;
    pub fn kmc_finalize_async(ctx: *mut KmcCtx) -> c_int;
    pub fn kmc_read_peak_device(d_buf: *const c_void, n_bytes: u64, device: c_int, stream: *mut c_void, shape: c_int, iters: c_int, ms_avg: *mut f64, xor_out: *mut u64) -> c_int;
    pub fn kmc_read_pieces(read_len: u64, k: c_int, starts: *mut u64, ends: *mut u64, cap: u64) -> u64;
    pub fn kmc_forget_source(ctx: *mut KmcCtx, what: c_int) -> c_int;
    pub fn kmc_get_stats(ctx: *const KmcCtx, out: *mut KmcStats) -> c_int;
    pub fn kmc_count_file(ctx: *mut KmcCtx, path: *const c_char, n_distinct: *mut u64, n_total: *mut u64) -> c_int;
    pub fn kmc_count_file_multi(ctxs: *mut *mut KmcCtx, n_ctx: u32, path: *const c_char, n_distinct: *mut u64, n_total: *mut u64) -> c_int;
    // host reader: whole file, or streaming (chunks end at record boundaries; buffers owned by the stream)
    pub fn kmc_parse_fasta(path: *const c_char, out: *mut KmcReads, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn kmc_free_reads(r: *mut KmcReads);
    pub fn kmc_fasta_stream_open(path: *const c_char, chunk_bytes: u64, out: *mut *mut KmcFastaStream, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn kmc_fasta_stream_next(s: *mut KmcFastaStream, out: *mut KmcReads, eof: *mut c_int, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn kmc_fasta_stream_close(s: *mut KmcFastaStream);
    pub fn kmc_decode_key(key_hi: u64, key_lo: u64, klen: c_int, out: *mut c_char);
    // seeded re-creation of random_fasta_generator.py's distribution
    pub fn kmc_synth_records_for_bytes(s: *const KmcSynth, file_bytes: u64, exact_bytes: *mut u64) -> u64;
    pub fn kmc_synth_reads_host(s: *const KmcSynth, first_record: u64, n_records: u64, bases: *mut u8, offsets: *mut u64) -> c_int;
    pub fn kmc_synth_reads_device(s: *const KmcSynth, first_record: u64, n_records: u64, d_bases: *mut c_void, d_offsets: *mut c_void, device: c_int, stream: *mut c_void) -> c_int;
    pub fn kmc_synth_write_fasta(s: *const KmcSynth, first_record: u64, n_records: u64, FILE_ptr: *mut c_void) -> c_int;
}

/// One counting context on one GPU.  Not `Sync`: a ctx is single-threaded (kmc.h).
pub struct Counter {
    ctx: *mut KmcCtx,
    klen: i32,
}

#[derive(Debug)]
pub struct KmcError(pub i32, pub String);

impl Counter {
    /// `k = None` is the reference's own computation (27 + gap + 27, sizes 80..=140, main.rs:48-49,63).
    pub fn new(k: Option<i32>, canonical: bool, device: i32) -> Result<Counter, KmcError> {
        let cfg = KmcConfig {
            struct_size: std::mem::size_of::<KmcConfig>() as u32,
            k: k.unwrap_or(54),
            mode: if k.is_some() { KMC_MODE_CONTIG } else { KMC_MODE_LR },
            canonical: canonical as i32,
            device,
            algo: KMC_ALGO_AUTO,
            capacity_hint: 0,
            stream: std::ptr::null_mut(),
        };
        let mut ctx = std::ptr::null_mut();
        let rc = unsafe { kmc_create(&mut ctx, &cfg) };
        if rc != 0 {
            let msg = unsafe { CStr::from_ptr(kmc_last_error(std::ptr::null())) }.to_string_lossy().into_owned();
            return Err(KmcError(rc, msg));
        }
        Ok(Counter { ctx, klen: k.unwrap_or(54) })
    }

    fn check(&self, rc: c_int) -> Result<(), KmcError> {
        if rc == 0 {
            return Ok(());
        }
        let msg = unsafe { CStr::from_ptr(kmc_last_error(self.ctx)) }.to_string_lossy().into_owned();
        Err(KmcError(rc, msg))
    }

    /// `bases`: all reads concatenated; `offsets[n_reads+1]`.  Buffers are free again on return.
    pub fn add_batch(&mut self, bases: &[u8], offsets: &[u64]) -> Result<(), KmcError> {
        if offsets.is_empty() {
            return Err(KmcError(-1, "offsets must hold n_reads + 1 entries (at least one)".into()));
        }
        let rc = unsafe { kmc_add_batch(self.ctx, bases.as_ptr(), offsets.as_ptr(), (offsets.len() - 1) as u64) };
        self.check(rc)
    }

    /// FASTA path in: the library's own pipelined reader (parse on the host cores overlapped with
    /// upload and counting) instead of `bio`'s record loop (main.rs:44-46,58-62).
    pub fn count_file(&mut self, path: &str) -> Result<(u64, u64), KmcError> {
        let c = std::ffi::CString::new(path).map_err(|_| KmcError(-1, "path contains NUL".into()))?;
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_count_file(self.ctx, c.as_ptr(), &mut nd, &mut nt) })?;
        Ok((nd, nt))
    }

    /// Sorted table: (key as ASCII, count), ascending == the order of `lr_chunk.sort()` (main.rs:87).
    pub fn table(&mut self) -> Result<Vec<(String, u64)>, KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let n = nd as usize;
        let (mut hi, mut lo, mut cnt) = (vec![0u64; n], vec![0u64; n], vec![0u64; n]);
        self.check(unsafe { kmc_export(self.ctx, hi.as_mut_ptr(), lo.as_mut_ptr(), cnt.as_mut_ptr(), nd) })?;
        let mut buf = vec![0u8; self.klen as usize];
        let mut out = Vec::with_capacity(n);
        for i in 0..n {
            unsafe { kmc_decode_key(hi[i], lo[i], self.klen, buf.as_mut_ptr() as *mut c_char) };
            out.push((String::from_utf8_lossy(&buf).into_owned(), cnt[i]));
        }
        Ok(out)
    }

    /// Abundance histogram of the table (`hist[c]` = keys seen `c` times, the last bin `>= n_bins - 1`), counting only
    /// keys with `min_count <= count <= max_count` (`max_count` 0: no upper bound), and the largest such count.
    pub fn histogram(&mut self, n_bins: u32, min_count: u64, max_count: u64) -> Result<(Vec<u64>, u64), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let mut hist = vec![0u64; n_bins as usize];
        let mut max_seen = 0u64;
        self.check(unsafe { kmc_histogram(self.ctx, min_count, max_count, n_bins, hist.as_mut_ptr(), &mut max_seen) })?;
        Ok((hist, max_seen))
    }

    /// `table()` restricted to keys with `min_count <= count <= max_count` (`max_count` 0: no upper bound), same order.
    pub fn table_filtered(&mut self, min_count: u64, max_count: u64) -> Result<Vec<(String, u64)>, KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let mut n = 0u64;
        let rc = unsafe {
            kmc_export_filtered(self.ctx, min_count, max_count, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut n)
        };
        if rc != 0 && n == 0 {
            self.check(rc)?;
        }
        let k = n as usize;
        let (mut hi, mut lo, mut cnt) = (vec![0u64; k], vec![0u64; k], vec![0u64; k]);
        if k > 0 {
            self.check(unsafe { kmc_export_filtered(self.ctx, min_count, max_count, hi.as_mut_ptr(), lo.as_mut_ptr(), cnt.as_mut_ptr(), n, &mut n) })?;
        }
        let mut buf = vec![0u8; self.klen as usize];
        let mut out = Vec::with_capacity(k);
        for i in 0..k {
            unsafe { kmc_decode_key(hi[i], lo[i], self.klen, buf.as_mut_ptr() as *mut c_char) };
            out.push((String::from_utf8_lossy(&buf).into_owned(), cnt[i]));
        }
        Ok(out)
    }

    /// Counts of the given packed keys in the table (0 = absent), looked up as given (`kmc_query`); `key_hi` may be
    /// empty when the keys fit one word.
    pub fn query(&mut self, key_hi: &[u64], key_lo: &[u64]) -> Result<Vec<u64>, KmcError> {
        if !key_hi.is_empty() && key_hi.len() != key_lo.len() {
            return Err(KmcError(-1, "key_hi and key_lo differ in length".into()));
        }
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let mut count = vec![0u64; key_lo.len()];
        let hi = if key_hi.is_empty() { std::ptr::null() } else { key_hi.as_ptr() };
        self.check(unsafe { kmc_query(self.ctx, hi, key_lo.as_ptr(), key_lo.len() as u64, count.as_mut_ptr()) })?;
        Ok(count)
    }

    /// Per-read k-mer profile of a batch against the table (`kmc_profile`; the batch is not counted): the count of the
    /// window starting at every base (saturated u32) and, per read, [valid windows, windows with count >=
    /// max(min_count, 1), min, max, sum].
    pub fn profile(&mut self, bases: &[u8], offsets: &[u64], min_count: u64) -> Result<(Vec<u32>, Vec<[u64; KMC_PROFILE_WORDS]>), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let n_reads = offsets.len().saturating_sub(1);
        if n_reads > 0 && offsets[n_reads] as usize != bases.len() {
            return Err(KmcError(-1, "offsets do not end at the number of bases".into()));
        }
        let mut win = vec![0u32; bases.len()];
        let mut stats = vec![[0u64; KMC_PROFILE_WORDS]; n_reads];
        self.check(unsafe {
            kmc_profile(self.ctx, bases.as_ptr(), offsets.as_ptr(), n_reads as u64, min_count, win.as_mut_ptr(), stats.as_mut_ptr() as *mut u64)
        })?;
        Ok((win, stats))
    }

    /// The eight words of `kmc_compare` for this table (A) and `other` (B), counts restricted to `range_a` / `range_b`
    /// = (min, max), max 0: no upper bound.  [n_a, n_b, n_both, sum_a, sum_b, shared_sum_a, shared_sum_b, sum_min];
    /// Jaccard is `w[2] / (w[0] + w[1] - w[2])`, weighted Jaccard `w[7] / (w[3] + w[4] - w[7])`.
    pub fn compare(&mut self, other: &mut Counter, range_a: (u64, u64), range_b: (u64, u64)) -> Result<[u64; KMC_COMPARE_WORDS], KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        other.check(unsafe { kmc_finalize(other.ctx, &mut nd, &mut nt) })?;
        let mut w = [0u64; KMC_COMPARE_WORDS];
        self.check(unsafe { kmc_compare(self.ctx, other.ctx, range_a.0, range_a.1, range_b.0, range_b.1, w.as_mut_ptr()) })?;
        Ok(w)
    }

    /// `self op other` (KMC_SETOP_*) with the result count given by `count_mode` (KMC_COUNT_*), sorted like `table()`.
    pub fn setop(&mut self, other: &mut Counter, op: i32, count_mode: i32, range_a: (u64, u64), range_b: (u64, u64)) -> Result<Vec<(String, u64)>, KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        other.check(unsafe { kmc_finalize(other.ctx, &mut nd, &mut nt) })?;
        let mut n = 0u64;
        let null = std::ptr::null_mut();
        let rc = unsafe { kmc_export_setop(self.ctx, other.ctx, op, count_mode, range_a.0, range_a.1, range_b.0, range_b.1, null, null, null, 0, &mut n) };
        if rc != 0 && n == 0 {
            self.check(rc)?;
        }
        let k = n as usize;
        let (mut hi, mut lo, mut cnt) = (vec![0u64; k], vec![0u64; k], vec![0u64; k]);
        if k > 0 {
            self.check(unsafe {
                kmc_export_setop(self.ctx, other.ctx, op, count_mode, range_a.0, range_a.1, range_b.0, range_b.1, hi.as_mut_ptr(), lo.as_mut_ptr(),
                                 cnt.as_mut_ptr(), n, &mut n)
            })?;
        }
        let mut buf = vec![0u8; self.klen as usize];
        let mut out = Vec::with_capacity(k);
        for i in 0..k {
            unsafe { kmc_decode_key(hi[i], lo[i], self.klen, buf.as_mut_ptr() as *mut c_char) };
            out.push((String::from_utf8_lossy(&buf).into_owned(), cnt[i]));
        }
        Ok(out)
    }

    /// The table as a de Bruijn graph (`kmc_graph`): one word per key of `table()`, in its order -- bits 0..3 the solid right
    /// extensions (ACGT), 4..7 the left ones, 8 / 9 "side R / L is a unitig end", 10 "the key is solid" -- and the eight
    /// summary words [nodes, R degrees, L degrees, isolated, dead ends, branching, end sides, single-node unitigs].  Solid:
    /// `min_count <= count <= max_count` (`max_count` 0: no upper bound).
    pub fn graph(&mut self, min_count: u64, max_count: u64) -> Result<(Vec<u16>, [u64; KMC_GRAPH_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let mut adj = vec![0u16; nd as usize];
        let mut w = [0u64; KMC_GRAPH_WORDS];
        let mut n = 0u64;
        self.check(unsafe { kmc_graph(self.ctx, min_count, max_count, adj.as_mut_ptr() as *mut c_void, nd, &mut n, w.as_mut_ptr()) })?;
        Ok((adj, w))
    }

    /// The unitigs of that graph (`kmc_unitigs`), in order: (sequence, summed count of its keys, circular) per unitig, and
    /// the eight summary words [unitigs, bases, keys, circular, one-key, keys of the longest, unjoined sides, abundance].
    pub fn unitigs(&mut self, min_count: u64, max_count: u64) -> Result<(Vec<(String, u64, bool)>, [u64; KMC_UNITIG_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let (mut nu, mut nb) = (0u64, 0u64);
        let mut w = [0u64; KMC_UNITIG_WORDS];
        let null8 = std::ptr::null_mut::<u8>();
        let null64 = std::ptr::null_mut::<u64>();
        self.check(unsafe { kmc_unitigs(self.ctx, min_count, max_count, null8, 0, null64, null64, null8, 0, &mut nu, &mut nb, w.as_mut_ptr()) })?;
        let mut bases = vec![0u8; nb as usize];
        let mut offsets = vec![0u64; nu as usize + 1];
        let mut abund = vec![0u64; nu as usize];
        let mut flags = vec![0u8; nu as usize];
        self.check(unsafe {
            kmc_unitigs(self.ctx, min_count, max_count, bases.as_mut_ptr(), nb, offsets.as_mut_ptr(), abund.as_mut_ptr(), flags.as_mut_ptr(), nu,
                        &mut nu, &mut nb, w.as_mut_ptr())
        })?;
        let mut out = Vec::with_capacity(nu as usize);
        for u in 0..nu as usize {
            let s = String::from_utf8_lossy(&bases[offsets[u] as usize..offsets[u + 1] as usize]).into_owned();
            out.push((s, abund[u], flags[u] & KMC_UNITIG_CIRCULAR != 0));
        }
        Ok((out, w))
    }

    /// The links between those unitigs (`kmc_unitig_links`): `offsets[2 n + 1]` indexed by unitig end (2u: the START end of
    /// unitig u, 2u + 1: its END end), the target ends of the records, and the eight summary words [unitigs, records, ends
    /// without a record, ends with two or more, self records, dropped, isolated unitigs, most records at one end].  Called
    /// after `unitigs` with the same range it does not compute the unitigs again.
    pub fn unitig_links(&mut self, min_count: u64, max_count: u64) -> Result<(Vec<u64>, Vec<u32>, [u64; KMC_LINK_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let (mut nu, mut nl) = (0u64, 0u64);
        let mut w = [0u64; KMC_LINK_WORDS];
        self.check(unsafe {
            kmc_unitig_links(self.ctx, min_count, max_count, std::ptr::null_mut::<u64>(), 0, std::ptr::null_mut::<u32>(), 0, &mut nu, &mut nl, w.as_mut_ptr())
        })?;
        let mut offsets = vec![0u64; 2 * nu as usize + 1];
        let mut to = vec![0u32; nl as usize];
        self.check(unsafe {
            kmc_unitig_links(self.ctx, min_count, max_count, offsets.as_mut_ptr(), 2 * nu, to.as_mut_ptr(), nl, &mut nu, &mut nl, w.as_mut_ptr())
        })?;
        Ok((offsets, to, w))
    }

    /// A batch of reads threaded through those unitigs (`kmc_unitig_map`; the batch is not counted).  Returns the place
    /// word of every base position (low half `2 * unitig + orientation` or `KMC_MAP_NONE`, high half the key position),
    /// per read [valid windows, placed windows, segments, crossings], `seg_offsets[n_reads + 1]`, the segments as
    /// [start, len, 2 * unitig + orientation, pos], the placed windows per unitig, and the eight summary words.  The host
    /// form of the library computes on every call, so the sizing call below maps the batch once more.
    #[allow(clippy::type_complexity)]
    pub fn map_reads(&mut self, bases: &[u8], offsets: &[u64], min_count: u64, max_count: u64)
                     -> Result<(Vec<u64>, Vec<[u32; KMC_MAP_READ_WORDS]>, Vec<u64>, Vec<[u32; 4]>, Vec<u64>, [u64; KMC_MAP_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let n_reads = offsets.len().saturating_sub(1);
        if n_reads > 0 && offsets[n_reads] as usize != bases.len() {
            return Err(KmcError(-1, "offsets do not end at the number of bases".into()));
        }
        let n_bases = if n_reads > 0 { bases.len() } else { 0 };
        let (mut ns, mut nu) = (0u64, 0u64);
        let mut w = [0u64; KMC_MAP_WORDS];
        let mut place = vec![0u64; n_bases];
        let mut stats = vec![[0u32; KMC_MAP_READ_WORDS]; n_reads];
        let mut seg_offsets = vec![0u64; n_reads + 1];
        self.check(unsafe {
            kmc_unitig_map(self.ctx, min_count, max_count, bases.as_ptr(), offsets.as_ptr(), n_reads as u64, place.as_mut_ptr(),
                           stats.as_mut_ptr() as *mut u32, seg_offsets.as_mut_ptr(), std::ptr::null_mut::<u32>(), 0,
                           std::ptr::null_mut::<u64>(), 0, &mut ns, &mut nu, w.as_mut_ptr())
        })?;
        let mut segs = vec![[0u32; 4]; ns as usize];
        let mut support = vec![0u64; nu as usize];
        if ns > 0 || nu > 0 {
            self.check(unsafe {
                kmc_unitig_map(self.ctx, min_count, max_count, bases.as_ptr(), offsets.as_ptr(), n_reads as u64, std::ptr::null_mut::<u64>(),
                               std::ptr::null_mut::<u32>(), std::ptr::null_mut::<u64>(), segs.as_mut_ptr() as *mut u32, ns,
                               support.as_mut_ptr(), nu, &mut ns, &mut nu, w.as_mut_ptr())
            })?;
        }
        Ok((place, stats, seg_offsets, segs, support, w))
    }

    /// The read walks of a batch counted per graph element (`kmc_unitig_transits`; the batch is not counted).  Returns the
    /// support of every link record (indexed like the `to` of `unitig_links`), `transit_offsets[n_unitigs + 1]`, the transit
    /// slots (unitig u: a dS x dE matrix at its offset, row = record rank at the START end, column = at the END end), the
    /// verdict per unitig (`KMC_TRANSIT_*`) and the eight summary words [crossings, those without a record, records without
    /// support, transits stored, dropped, repeats, resolved, ambiguous].  `accumulate` adds onto the result of the last call
    /// for this range (the first batch goes without it).  The arrays are sized from `kmc_unitig_links` -- a unitig's slots
    /// are at most four times the records of one of its ends -- so the batch is walked once.
    #[allow(clippy::type_complexity)]
    pub fn transits(&mut self, bases: &[u8], offsets: &[u64], min_count: u64, max_count: u64, min_reads: u64, accumulate: bool)
                    -> Result<(Vec<u64>, Vec<u64>, Vec<u64>, Vec<u8>, [u64; KMC_TRANSIT_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let n_reads = offsets.len().saturating_sub(1);
        if n_reads > 0 && offsets[n_reads] as usize != bases.len() {
            return Err(KmcError(-1, "offsets do not end at the number of bases".into()));
        }
        let (mut nu, mut nl, mut nsl) = (0u64, 0u64, 0u64);
        let mut lw = [0u64; KMC_LINK_WORDS];
        self.check(unsafe {
            kmc_unitig_links(self.ctx, min_count, max_count, std::ptr::null_mut::<u64>(), 0, std::ptr::null_mut::<u32>(), 0, &mut nu, &mut nl, lw.as_mut_ptr())
        })?;
        let cap_slots = std::cmp::min(16 * nu, 4 * nl);
        let mut support = vec![0u64; nl as usize];
        let mut transit_offsets = vec![0u64; nu as usize + 1];
        let mut count = vec![0u64; cap_slots as usize];
        let mut verdict = vec![0u8; nu as usize];
        let mut w = [0u64; KMC_TRANSIT_WORDS];
        self.check(unsafe {
            kmc_unitig_transits(self.ctx, min_count, max_count, min_reads, if accumulate { KMC_TRANSIT_ACCUMULATE } else { 0 }, bases.as_ptr(),
                                offsets.as_ptr(), n_reads as u64, support.as_mut_ptr(), nl, transit_offsets.as_mut_ptr(), nu, count.as_mut_ptr(),
                                cap_slots, verdict.as_mut_ptr(), &mut nu, &mut nl, &mut nsl, w.as_mut_ptr())
        })?;
        count.truncate(nsl as usize);
        Ok((support, transit_offsets, count, verdict, w))
    }

    /// The pair evidence of a batch of interleaved mates (`kmc_unitig_pairs`; reads 2i and 2i + 1 are pair i, forward /
    /// reverse; the batch is not counted).  Returns per pair the class (`KMC_PAIR_*`), the two out ends and the value (R of a
    /// SPAN pair, the insert size of a PROPER one), per record in ascending (a, b) the two ends, count, sum, min and max of R,
    /// the insert histogram of `n_bins` bins (the last one open) and the eight summary words [pairs, unplaced, span, proper,
    /// everted, same strand, records, sum of the insert sizes].  `accumulate` adds the records, the histogram and the words
    /// onto the result of the last call for this range and `n_bins` (the first batch goes without it).  `held_records` is the
    /// number of records the last call returned (0 without `accumulate`): there are at most that many more than pairs.
    #[allow(clippy::type_complexity)]
    pub fn pairs(&mut self, bases: &[u8], offsets: &[u64], min_count: u64, max_count: u64, n_bins: u64, accumulate: bool, held_records: u64)
                 -> Result<(Vec<u8>, Vec<u32>, Vec<u64>, Vec<u32>, Vec<u64>, Vec<u64>, Vec<u64>, Vec<u64>, Vec<u64>, [u64; KMC_PAIR_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let n_reads = offsets.len().saturating_sub(1);
        if n_reads > 0 && offsets[n_reads] as usize != bases.len() {
            return Err(KmcError(-1, "offsets do not end at the number of bases".into()));
        }
        let cap_pairs = (n_reads / 2) as u64;
        let cap_records = cap_pairs + if accumulate { held_records } else { 0 };
        let mut class = vec![0u8; cap_pairs as usize];
        let mut ends = vec![0u32; 2 * cap_pairs as usize];
        let mut value = vec![0u64; cap_pairs as usize];
        let mut rec_ends = vec![0u32; 2 * cap_records as usize];
        let mut rec = [vec![0u64; cap_records as usize], vec![0u64; cap_records as usize], vec![0u64; cap_records as usize], vec![0u64; cap_records as usize]];
        let mut hist = vec![0u64; n_bins as usize];
        let (mut np, mut nr) = (0u64, 0u64);
        let mut w = [0u64; KMC_PAIR_WORDS];
        let [rc, rs, rn, rx] = &mut rec;
        self.check(unsafe {
            kmc_unitig_pairs(self.ctx, min_count, max_count, n_bins, if accumulate { KMC_PAIR_ACCUMULATE } else { 0 }, bases.as_ptr(), offsets.as_ptr(),
                             n_reads as u64, class.as_mut_ptr(), ends.as_mut_ptr(), value.as_mut_ptr(), cap_pairs, rec_ends.as_mut_ptr(), rc.as_mut_ptr(),
                             rs.as_mut_ptr(), rn.as_mut_ptr(), rx.as_mut_ptr(), cap_records, hist.as_mut_ptr(), n_bins, &mut np, &mut nr, w.as_mut_ptr())
        })?;
        rec_ends.truncate(2 * nr as usize);
        let [mut rc, mut rs, mut rn, mut rx] = rec;
        for v in [&mut rc, &mut rs, &mut rn, &mut rx] {
            v.truncate(nr as usize);
        }
        Ok((class, ends, value, rec_ends, rc, rs, rn, rx, hist, w))
    }

    /// The contigs of the counted walks (`kmc_unitig_contigs`): behind a `transits` call of the same range, every repeat its
    /// counts resolve under `min_reads` has one copy per matched way through it, records below `min_support` are ignored at
    /// the ends of single-copy unitigs (0: none is), and the chains that remain are spelled out.  Returns the bases
    /// (concatenated), `offsets[n_contigs + 1]`, `path_offsets[n_contigs + 1]`, the path entries `2 * unitig + o` (o = 1: read
    /// reverse-complemented), the abundance per contig (a duplicated repeat counts in full in each copy), the flags (bit 0:
    /// circular) and the eight summary words [contigs, nodes, unitigs duplicated, records ignored, circular, one-node, most
    /// nodes in one, bases].  A sizing call, then the copy call: the library computes once.
    #[allow(clippy::type_complexity)]
    pub fn contigs(&mut self, min_count: u64, max_count: u64, min_reads: u64, min_support: u64)
                   -> Result<(Vec<u8>, Vec<u64>, Vec<u64>, Vec<u32>, Vec<u64>, Vec<u8>, [u64; KMC_CONTIG_WORDS]), KmcError> {
        let (mut nc, mut nn, mut nb) = (0u64, 0u64, 0u64);
        let mut w = [0u64; KMC_CONTIG_WORDS];
        self.check(unsafe {
            kmc_unitig_contigs(self.ctx, min_count, max_count, min_reads, min_support, std::ptr::null_mut::<u8>(), 0, std::ptr::null_mut::<u64>(),
                               std::ptr::null_mut::<u64>(), std::ptr::null_mut::<u64>(), std::ptr::null_mut::<u8>(), 0, std::ptr::null_mut::<u32>(), 0,
                               &mut nc, &mut nn, &mut nb, w.as_mut_ptr())
        })?;
        let mut bases = vec![0u8; nb as usize];
        let mut offsets = vec![0u64; nc as usize + 1];
        let mut path_offsets = vec![0u64; nc as usize + 1];
        let mut path = vec![0u32; nn as usize];
        let mut abund = vec![0u64; nc as usize];
        let mut flags = vec![0u8; nc as usize];
        self.check(unsafe {
            kmc_unitig_contigs(self.ctx, min_count, max_count, min_reads, min_support, bases.as_mut_ptr(), nb, offsets.as_mut_ptr(),
                               path_offsets.as_mut_ptr(), abund.as_mut_ptr(), flags.as_mut_ptr(), nc, path.as_mut_ptr(), nn, &mut nc, &mut nn, &mut nb,
                               w.as_mut_ptr())
        })?;
        Ok((bases, offsets, path_offsets, path, abund, flags, w))
    }

    /// A batch of reads corrected against the solid keys of the table (`kmc_correct`; the batch is not counted): every
    /// substitution error that leaves one clean run of weak windows is replaced by the one base that makes all windows
    /// over it solid.  Returns the corrected bases (the offsets are the caller's), per read [valid windows, weak windows,
    /// candidates, corrected], `cand_offsets[n_reads + 1]`, the candidates as [p, old | new << 8 | kind << 16 | accepted
    /// mask << 24, a, n], and the eight summary words.  The host form computes on every call, so the sizing call below
    /// corrects the batch once more.
    #[allow(clippy::type_complexity)]
    pub fn correct_reads(&mut self, bases: &[u8], offsets: &[u64], min_count: u64, max_count: u64)
                         -> Result<(Vec<u8>, Vec<[u32; KMC_CORRECT_READ_WORDS]>, Vec<u64>, Vec<[u32; 4]>, [u64; KMC_CORRECT_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let n_reads = offsets.len().saturating_sub(1);
        if n_reads > 0 && offsets[n_reads] as usize != bases.len() {
            return Err(KmcError(-1, "offsets do not end at the number of bases".into()));
        }
        let n_bases = if n_reads > 0 { bases.len() } else { 0 };
        let mut nc = 0u64;
        let mut w = [0u64; KMC_CORRECT_WORDS];
        let mut out = vec![0u8; n_bases];
        let mut stats = vec![[0u32; KMC_CORRECT_READ_WORDS]; n_reads];
        let mut cand_offsets = vec![0u64; n_reads + 1];
        self.check(unsafe {
            kmc_correct(self.ctx, min_count, max_count, bases.as_ptr(), offsets.as_ptr(), n_reads as u64, out.as_mut_ptr(),
                        stats.as_mut_ptr() as *mut u32, cand_offsets.as_mut_ptr(), std::ptr::null_mut::<u32>(), 0, &mut nc, w.as_mut_ptr())
        })?;
        let mut cands = vec![[0u32; 4]; nc as usize];
        if nc > 0 {
            self.check(unsafe {
                kmc_correct(self.ctx, min_count, max_count, bases.as_ptr(), offsets.as_ptr(), n_reads as u64, std::ptr::null_mut::<u8>(),
                            std::ptr::null_mut::<u32>(), std::ptr::null_mut::<u64>(), cands.as_mut_ptr() as *mut u32, nc, &mut nc, w.as_mut_ptr())
            })?;
        }
        Ok((out, stats, cand_offsets, cands, w))
    }

    /// A batch of reads trimmed and filtered by their strong windows (`kmc_trim`; the batch is not counted).  `mode`: the
    /// span of a read (`KMC_TRIM_NONE` the whole read, `KMC_TRIM_ENDS` from its first to its last strong window,
    /// `KMC_TRIM_LONGEST` its longest run of strong windows); a read passes with `min_strong` strong windows,
    /// `min_permille` thousandths of its valid windows strong and a span of `min_len` bases; `flags`: `KMC_TRIM_INVERT`,
    /// `KMC_TRIM_PAIR_BOTH`, `KMC_TRIM_PAIR_EITHER`.  Returns the emitted spans as a batch (bases, offsets), the source read
    /// of each, per read of the input [valid windows, strong windows, span start, span length] and the verdict byte, and
    /// the eight summary words.  The host form computes on every call, so the sizing call below judges the batch once more.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn trim_reads(&mut self, bases: &[u8], offsets: &[u64], min_count: u64, max_count: u64, mode: c_int, flags: u32, min_strong: u64,
                      min_permille: u32, min_len: u64)
                      -> Result<(Vec<u8>, Vec<u64>, Vec<u64>, Vec<[u32; KMC_TRIM_READ_WORDS]>, Vec<u8>, [u64; KMC_TRIM_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let n_reads = offsets.len().saturating_sub(1);
        if n_reads > 0 && offsets[n_reads] as usize != bases.len() {
            return Err(KmcError(-1, "offsets do not end at the number of bases".into()));
        }
        let (mut no, mut nb) = (0u64, 0u64);
        let mut w = [0u64; KMC_TRIM_WORDS];
        let mut stats = vec![[0u32; KMC_TRIM_READ_WORDS]; n_reads];
        let mut verdict = vec![0u8; n_reads];
        self.check(unsafe {
            kmc_trim(self.ctx, min_count, max_count, mode, flags, min_strong, min_permille, min_len, bases.as_ptr(), offsets.as_ptr(),
                     n_reads as u64, std::ptr::null_mut::<u8>(), 0, std::ptr::null_mut::<u64>(), std::ptr::null_mut::<u64>(), 0,
                     stats.as_mut_ptr() as *mut u32, verdict.as_mut_ptr(), &mut no, &mut nb, w.as_mut_ptr())
        })?;
        let mut out = vec![0u8; nb as usize];
        let mut out_offsets = vec![0u64; no as usize + 1];
        let mut origin = vec![0u64; no as usize];
        self.check(unsafe {
            kmc_trim(self.ctx, min_count, max_count, mode, flags, min_strong, min_permille, min_len, bases.as_ptr(), offsets.as_ptr(),
                     n_reads as u64, out.as_mut_ptr(), nb, out_offsets.as_mut_ptr(), origin.as_mut_ptr(), no, std::ptr::null_mut::<u32>(),
                     std::ptr::null_mut::<u8>(), &mut no, &mut nb, w.as_mut_ptr())
        })?;
        Ok((out, out_offsets, origin, stats, verdict, w))
    }

    /// A batch of reads normalised by depth (`kmc_normalize`; the batch is not counted).  A read's depth is the count at
    /// `permille` thousandths (500: the lower median) of the sorted counts of its valid windows; a unit -- a read, or with
    /// `KMC_NORM_PAIRED` a pair judged by its smaller depth -- below `min_depth` is dropped, one above `target` is kept with
    /// probability `target / depth` by a draw from `seed` and the unit's number (`target` 0: nothing is sampled down);
    /// `KMC_NORM_INVERT` emits the others.  Returns the emitted reads whole as a batch (bases, offsets), the source read of
    /// each, per read of the input [valid windows, own depth, unit depth, draw] and the verdict byte (`KMC_NORM_KEEP`,
    /// `KMC_NORM_EMITTED`, `KMC_NORM_LOW`, `KMC_NORM_DEEP`), and the eight summary words.  The host form computes on every
    /// call, so the sizing call below judges the batch once more.
    #[allow(clippy::type_complexity, clippy::too_many_arguments)]
    pub fn normalize_reads(&mut self, bases: &[u8], offsets: &[u64], permille: u32, target: u64, min_depth: u64, seed: u64, flags: u32)
                           -> Result<(Vec<u8>, Vec<u64>, Vec<u64>, Vec<[u32; KMC_NORMALIZE_READ_WORDS]>, Vec<u8>, [u64; KMC_NORMALIZE_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let n_reads = offsets.len().saturating_sub(1);
        if n_reads > 0 && offsets[n_reads] as usize != bases.len() {
            return Err(KmcError(-1, "offsets do not end at the number of bases".into()));
        }
        let (mut no, mut nb) = (0u64, 0u64);
        let mut w = [0u64; KMC_NORMALIZE_WORDS];
        let mut stats = vec![[0u32; KMC_NORMALIZE_READ_WORDS]; n_reads];
        let mut verdict = vec![0u8; n_reads];
        self.check(unsafe {
            kmc_normalize(self.ctx, permille, target, min_depth, seed, flags, bases.as_ptr(), offsets.as_ptr(), n_reads as u64,
                          std::ptr::null_mut::<u8>(), 0, std::ptr::null_mut::<u64>(), std::ptr::null_mut::<u64>(), 0,
                          stats.as_mut_ptr() as *mut u32, verdict.as_mut_ptr(), &mut no, &mut nb, w.as_mut_ptr())
        })?;
        let mut out = vec![0u8; nb as usize];
        let mut out_offsets = vec![0u64; no as usize + 1];
        let mut origin = vec![0u64; no as usize];
        self.check(unsafe {
            kmc_normalize(self.ctx, permille, target, min_depth, seed, flags, bases.as_ptr(), offsets.as_ptr(), n_reads as u64,
                          out.as_mut_ptr(), nb, out_offsets.as_mut_ptr(), origin.as_mut_ptr(), no, std::ptr::null_mut::<u32>(),
                          std::ptr::null_mut::<u8>(), &mut no, &mut nb, w.as_mut_ptr())
        })?;
        Ok((out, out_offsets, origin, stats, verdict, w))
    }

    /// That graph cleaned (`kmc_unitig_clean`): the keys of the kept unitigs with their counts, in the order of `table()`,
    /// the verdict per unitig (`KMC_CLEAN_KEEP` / `KMC_CLEAN_TIP` / `KMC_CLEAN_ISLAND`, indexed as `unitigs` numbers them) and
    /// the eight summary words [unitigs, tips, islands, keys kept, keys of tips, keys of islands, tip candidates, sum of the
    /// kept counts].  A dead-end arm of at most `max_tip_keys` keys that loses against a sibling is a tip, an unconnected
    /// unitig of at most `max_island_keys` keys an island; 0 switches a rule off.
    pub fn clean_unitigs(&mut self, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64)
                         -> Result<(Vec<(String, u64)>, Vec<u8>, [u64; KMC_CLEAN_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let (mut nk, mut nu) = (0u64, 0u64);
        let mut w = [0u64; KMC_CLEAN_WORDS];
        let null64 = std::ptr::null_mut::<u64>();
        self.check(unsafe {
            kmc_unitig_clean(self.ctx, min_count, max_count, max_tip_keys, max_island_keys, null64, null64, null64, 0, std::ptr::null_mut::<u8>(), 0,
                             &mut nk, &mut nu, w.as_mut_ptr())
        })?;
        let k = nk as usize;
        let (mut hi, mut lo, mut cnt) = (vec![0u64; k], vec![0u64; k], vec![0u64; k]);
        let mut verdict = vec![0u8; nu as usize];
        self.check(unsafe {
            kmc_unitig_clean(self.ctx, min_count, max_count, max_tip_keys, max_island_keys, hi.as_mut_ptr(), lo.as_mut_ptr(), cnt.as_mut_ptr(), nk,
                             verdict.as_mut_ptr(), nu, &mut nk, &mut nu, w.as_mut_ptr())
        })?;
        let mut buf = vec![0u8; self.klen as usize];
        let mut out = Vec::with_capacity(k);
        for i in 0..k {
            unsafe { kmc_decode_key(hi[i], lo[i], self.klen, buf.as_mut_ptr() as *mut c_char) };
            out.push((String::from_utf8_lossy(&buf).into_owned(), cnt[i]));
        }
        Ok((out, verdict, w))
    }

    /// One step of a cleaning round (`kmc_unitig_clean_into`): the keys of the kept unitigs of `self` merged into the table
    /// of `dst`, another counter of the same k, strand rule and device.  `dst` is not finalized, so several sources can be
    /// merged; its `table()` is the cleaned table.  Returns the summary words of `clean_unitigs`.
    pub fn clean_into(&mut self, dst: &mut Counter, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64)
                      -> Result<[u64; KMC_CLEAN_WORDS], KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let mut w = [0u64; KMC_CLEAN_WORDS];
        self.check(unsafe { kmc_unitig_clean_into(self.ctx, dst.ctx, min_count, max_count, max_tip_keys, max_island_keys, w.as_mut_ptr()) })?;
        Ok(w)
    }

    /// `clean_unitigs` with simple bubbles popped (`kmc_unitig_simplify`): a unitig of at most `max_bubble_keys` keys with one
    /// link at each end that loses against a parallel unitig between the same two ends gets `KMC_CLEAN_BUBBLE`; 0 pops
    /// nothing.  Twelve summary words: those of `clean_unitigs`, then [bubbles, their keys, bubble candidates, the sum of
    /// the counts of their keys].  The counts of a popped arm are not added to the survivor.
    pub fn simplify_unitigs(&mut self, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64, max_bubble_keys: u64)
                            -> Result<(Vec<(String, u64)>, Vec<u8>, [u64; KMC_SIMPLIFY_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let (mut nk, mut nu) = (0u64, 0u64);
        let mut w = [0u64; KMC_SIMPLIFY_WORDS];
        let null64 = std::ptr::null_mut::<u64>();
        self.check(unsafe {
            kmc_unitig_simplify(self.ctx, min_count, max_count, max_tip_keys, max_island_keys, max_bubble_keys, null64, null64, null64, 0,
                                std::ptr::null_mut::<u8>(), 0, &mut nk, &mut nu, w.as_mut_ptr())
        })?;
        let k = nk as usize;
        let (mut hi, mut lo, mut cnt) = (vec![0u64; k], vec![0u64; k], vec![0u64; k]);
        let mut verdict = vec![0u8; nu as usize];
        self.check(unsafe {
            kmc_unitig_simplify(self.ctx, min_count, max_count, max_tip_keys, max_island_keys, max_bubble_keys, hi.as_mut_ptr(), lo.as_mut_ptr(),
                                cnt.as_mut_ptr(), nk, verdict.as_mut_ptr(), nu, &mut nk, &mut nu, w.as_mut_ptr())
        })?;
        let mut buf = vec![0u8; self.klen as usize];
        let mut out = Vec::with_capacity(k);
        for i in 0..k {
            unsafe { kmc_decode_key(hi[i], lo[i], self.klen, buf.as_mut_ptr() as *mut c_char) };
            out.push((String::from_utf8_lossy(&buf).into_owned(), cnt[i]));
        }
        Ok((out, verdict, w))
    }

    /// One step of a round that also pops bubbles (`kmc_unitig_simplify_into`): as `clean_into`, with the twelve words of
    /// `simplify_unitigs`.
    pub fn simplify_into(&mut self, dst: &mut Counter, min_count: u64, max_count: u64, max_tip_keys: u64, max_island_keys: u64,
                         max_bubble_keys: u64) -> Result<[u64; KMC_SIMPLIFY_WORDS], KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let mut w = [0u64; KMC_SIMPLIFY_WORDS];
        self.check(unsafe {
            kmc_unitig_simplify_into(self.ctx, dst.ctx, min_count, max_count, max_tip_keys, max_island_keys, max_bubble_keys, w.as_mut_ptr())
        })?;
        Ok(w)
    }

    /// The connected components of the unitig graph (`kmc_unitig_components`): the component of every unitig (numbered by
    /// their smallest unitig), `[root, unitigs, keys, abundance]` per component, the verdict per unitig (`KMC_CLEAN_KEEP`, or
    /// `KMC_CLEAN_COMPONENT` in a component of at most `max_component_keys` keys; 0 drops none), the kept table and the
    /// eight summary words.
    #[allow(clippy::type_complexity)]
    pub fn components(&mut self, min_count: u64, max_count: u64, max_component_keys: u64)
                      -> Result<(Vec<u32>, Vec<[u64; KMC_COMPONENT_STAT_WORDS]>, Vec<u8>, Vec<(String, u64)>, [u64; KMC_COMPONENT_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let (mut nc, mut nu, mut nk) = (0u64, 0u64, 0u64);
        let mut w = [0u64; KMC_COMPONENT_WORDS];
        let null64 = std::ptr::null_mut::<u64>();
        self.check(unsafe {
            kmc_unitig_components(self.ctx, min_count, max_count, max_component_keys, std::ptr::null_mut::<u32>(), std::ptr::null_mut::<u8>(), 0,
                                  null64, 0, null64, null64, null64, 0, &mut nc, &mut nu, &mut nk, w.as_mut_ptr())
        })?;
        let k = nk as usize;
        let (mut hi, mut lo, mut cnt) = (vec![0u64; k], vec![0u64; k], vec![0u64; k]);
        let mut comp_of = vec![0u32; nu as usize];
        let mut verdict = vec![0u8; nu as usize];
        let mut stats = vec![[0u64; KMC_COMPONENT_STAT_WORDS]; nc as usize];
        self.check(unsafe {
            kmc_unitig_components(self.ctx, min_count, max_count, max_component_keys, comp_of.as_mut_ptr(), verdict.as_mut_ptr(), nu,
                                  stats.as_mut_ptr() as *mut u64, nc, hi.as_mut_ptr(), lo.as_mut_ptr(), cnt.as_mut_ptr(), nk, &mut nc, &mut nu,
                                  &mut nk, w.as_mut_ptr())
        })?;
        let mut buf = vec![0u8; self.klen as usize];
        let mut out = Vec::with_capacity(k);
        for i in 0..k {
            unsafe { kmc_decode_key(hi[i], lo[i], self.klen, buf.as_mut_ptr() as *mut c_char) };
            out.push((String::from_utf8_lossy(&buf).into_owned(), cnt[i]));
        }
        Ok((comp_of, stats, verdict, out, w))
    }

    /// One step that drops small components (`kmc_unitig_components_into`): as `clean_into`, with the eight words of
    /// `components`.
    pub fn components_into(&mut self, dst: &mut Counter, min_count: u64, max_count: u64, max_component_keys: u64)
                           -> Result<[u64; KMC_COMPONENT_WORDS], KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let mut w = [0u64; KMC_COMPONENT_WORDS];
        self.check(unsafe { kmc_unitig_components_into(self.ctx, dst.ctx, min_count, max_count, max_component_keys, w.as_mut_ptr()) })?;
        Ok(w)
    }

    /// The bubbles of the unitig graph as variant records (`kmc_unitig_bubbles`): per unitig that loses against a parallel
    /// one, ascending, `[u, w, p, q, lcp, lcs, kind | KMC_BUBBLE_REVERSED, mism]`, and the eight summary words.
    /// `max_bubble_keys` is the most keys an arm may have (0: none; 2^31 or more is an argument error).
    pub fn bubbles(&mut self, min_count: u64, max_count: u64, max_bubble_keys: u64)
                   -> Result<(Vec<[u32; KMC_BUBBLE_RECORD_WORDS]>, [u64; KMC_BUBBLE_WORDS]), KmcError> {
        let (mut nd, mut nt) = (0u64, 0u64);
        self.check(unsafe { kmc_finalize(self.ctx, &mut nd, &mut nt) })?;
        let (mut nr, mut nu) = (0u64, 0u64);
        let mut w = [0u64; KMC_BUBBLE_WORDS];
        self.check(unsafe {
            kmc_unitig_bubbles(self.ctx, min_count, max_count, max_bubble_keys, std::ptr::null_mut::<u32>(), 0, &mut nr, &mut nu, w.as_mut_ptr())
        })?;
        let mut rec = vec![[0u32; KMC_BUBBLE_RECORD_WORDS]; nr as usize];
        self.check(unsafe {
            kmc_unitig_bubbles(self.ctx, min_count, max_count, max_bubble_keys, rec.as_mut_ptr() as *mut u32, nr, &mut nr, &mut nu, w.as_mut_ptr())
        })?;
        Ok((rec, w))
    }
}

impl Drop for Counter {
    fn drop(&mut self) {
        unsafe { kmc_destroy(self.ctx) }
    }
}
