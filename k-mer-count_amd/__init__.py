"""k-mer-count_amd -- Python host side of the MI355X k-mer counter.

A thin ctypes binding over the C ABI of ``libkmc.so`` (``include/kmc.h``).  Python is the
host language here because the reference's own toolchain (Rust) is absent from this image;
the names mirror the reference's pipeline, ``k-mer-count/src/main.rs:43-91`` and
``test.py:14-40``: a FASTA path goes in, a table sorted like ``lr_chunk.sort()``
(main.rs:87) comes out, printed one ``println!`` line per occurrence (main.rs:88-90) in
reference mode or ``KMER<TAB>COUNT`` in ``-k`` mode.

Import with ``importlib.import_module("k-mer-count_amd")`` (the directory name is the one the
project layout prescribes; it is not a Python identifier).

There is no CPU fallback anywhere in this package: every counting call goes through the HIP
kernels in ``libkmc.so`` and raises if the library or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
from dataclasses import dataclass
from typing import Iterable, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# KMC_LIB_PATH: load another build of the same ABI (same-box A/B runs of kernel variants; tools/ab_bench.sh)
LIB_PATH = os.environ.get("KMC_LIB_PATH") or os.path.join(_HERE, "libkmc.so")

MODE_CONTIG, MODE_LR = 0, 1
ALGO_AUTO, ALGO_STREAM, ALGO_WALK, ALGO_SORT = 0, 1, 2, 3

OK = 0
ERR_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_NOMEM, ERR_IO, ERR_FORMAT, ERR_ALPHABET, ERR_CAPACITY, ERR_STATE = range(-1, -10, -1)


class KmcError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libkmc status {status}: {message}")
        self.status = status
        self.message = message


class _Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_int32), ("mode", C.c_int32), ("canonical", C.c_int32),
                ("device", C.c_int32), ("algo", C.c_int32), ("capacity_hint", C.c_uint64), ("stream", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_kmers", C.c_uint64), ("n_distinct", C.c_uint64),
                ("table_capacity", C.c_uint64), ("n_spilled", C.c_uint64), ("n_batches", C.c_uint64),
                ("kernel_ms_last", C.c_double), ("kernel_ms_total", C.c_double), ("algo_last", C.c_int32),
                ("launches_last", C.c_int32), ("n_slabs_skipped", C.c_uint64), ("n_direct", C.c_uint64),
                ("kernel_ms_lifetime", C.c_double), ("launches_lifetime", C.c_uint64),
                ("n_async_ok", C.c_uint64), ("n_async_slabs_skipped", C.c_uint64), ("n_planner_stale", C.c_uint64),
                ("walk_uniform_launches", C.c_uint64), ("walk_plan_finalizes", C.c_uint64),
                ("walk_plan_builds", C.c_uint64)]


class _Reads(C.Structure):
    _fields_ = [("bases", C.POINTER(C.c_uint8)), ("offsets", C.POINTER(C.c_uint64)), ("n_reads", C.c_uint64),
                ("n_bases", C.c_uint64), ("max_read_len", C.c_uint64)]


class Synth(C.Structure):
    """Parameters of the synthetic-input generator (random_fasta_generator.py:5-15 distribution)."""
    _fields_ = [("seed", C.c_uint64), ("pool", C.c_uint32), ("line_len", C.c_uint32),
                ("lines_per_record", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, seed=1, pool=10, line_len=80, lines_per_record=5):
        super().__init__(seed, pool, line_len, lines_per_record, 0)

    @property
    def read_len(self) -> int:
        return self.line_len * self.lines_per_record


# every symbol include/kmc.h declares
ABI_SYMBOLS = [
    "kmc_version", "kmc_status_string", "kmc_create", "kmc_destroy", "kmc_last_error", "kmc_reset",
    "kmc_add_batch", "kmc_add_batch_device", "kmc_merge_pairs_device", "kmc_finalize", "kmc_export",
    "kmc_export_device", "kmc_partition_device", "kmc_owner_of", "kmc_get_stats", "kmc_count_file",
    "kmc_parse_fasta", "kmc_free_reads", "kmc_decode_key", "kmc_synth_records_for_bytes",
    "kmc_synth_reads_host", "kmc_synth_reads_device", "kmc_synth_write_fasta",
    "kmc_slab_words", "kmc_pack_slab_device", "kmc_merge_slabs_device", "kmc_forget_source",
    "kmc_fasta_stream_open", "kmc_fasta_stream_next", "kmc_fasta_stream_close", "kmc_poll",
    "kmc_count_file_multi", "kmc_read_pieces", "kmc_sync", "kmc_read_peak_device", "kmc_finalize_async",
    "kmc_histogram", "kmc_filter_device", "kmc_export_filtered",
    "kmc_encode_key", "kmc_query", "kmc_query_device", "kmc_profile", "kmc_profile_device",
    "kmc_compare", "kmc_setop_device", "kmc_export_setop",
    "kmc_graph", "kmc_graph_device",
    "kmc_unitigs", "kmc_unitigs_device",
    "kmc_unitig_links", "kmc_unitig_links_device",
    "kmc_unitig_clean", "kmc_unitig_clean_device", "kmc_unitig_clean_into",
    "kmc_unitig_simplify", "kmc_unitig_simplify_device", "kmc_unitig_simplify_into",
    "kmc_unitig_components", "kmc_unitig_components_device", "kmc_unitig_components_into",
    "kmc_unitig_bubbles", "kmc_unitig_bubbles_device",
    "kmc_unitig_map", "kmc_unitig_map_device",
    "kmc_unitig_transits", "kmc_unitig_transits_device",
    "kmc_unitig_contigs", "kmc_unitig_contigs_device",
    "kmc_unitig_pairs", "kmc_unitig_pairs_device",
    "kmc_correct", "kmc_correct_device",
    "kmc_trim", "kmc_trim_device",
    "kmc_normalize", "kmc_normalize_device",
]

PROFILE_WORDS = 5  # KMC_PROFILE_WORDS: valid windows, present windows, min, max, sum
COMPARE_WORDS = 8  # KMC_COMPARE_WORDS: n_a, n_b, n_both, sum_a, sum_b, shared_sum_a, shared_sum_b, sum_min
GRAPH_WORDS = 8    # KMC_GRAPH_WORDS: nodes, R degrees, L degrees, isolated, dead ends, branching, end sides, single-node unitigs
GRAPH_END_R, GRAPH_END_L, GRAPH_SOLID = 1 << 8, 1 << 9, 1 << 10   # bits of an adj word above the two neighbour nibbles (R: 0..3, L: 4..7)
UNITIG_WORDS = 8   # KMC_UNITIG_WORDS: unitigs, bases, keys, circular, one-key, keys of the longest, unjoined sides, abundance
UNITIG_CIRCULAR = 1  # KMC_UNITIG_CIRCULAR: bit 0 of a unitig's flags byte
LINK_WORDS = 8     # KMC_LINK_WORDS: unitigs, records, ends without / with several records, self records, dropped, isolated unitigs, most at one end
CLEAN_WORDS = 8    # KMC_CLEAN_WORDS: unitigs, tips, islands, keys kept / of tips / of islands, tip candidates, sum of the kept counts
CLEAN_KEEP, CLEAN_TIP, CLEAN_ISLAND = 0, 1, 2   # KMC_CLEAN_*: a unitig's verdict byte
SIMPLIFY_WORDS = 12  # KMC_SIMPLIFY_WORDS: the clean words, then bubbles, their keys, bubble candidates, the counts of their keys
CLEAN_BUBBLE = 3     # KMC_CLEAN_BUBBLE: the fourth verdict, of a simplify call
COMPONENT_WORDS = 8       # KMC_COMPONENT_WORDS: unitigs, components, those of one unitig, most keys / unitigs in one, small ones, keys kept, their counts
COMPONENT_STAT_WORDS = 4  # KMC_COMPONENT_STAT_WORDS: a component's root, unitigs, keys, abundance
CLEAN_COMPONENT = 4       # KMC_CLEAN_COMPONENT: the verdict of a unitig in a small component, of a components call
BUBBLE_WORDS = 8          # KMC_BUBBLE_WORDS: unitigs, records, bubble candidates, substitutions, indels, complex, reversed records, keys of the called arms
BUBBLE_RECORD_WORDS = 8   # KMC_BUBBLE_RECORD_WORDS: u, w, p, q, lcp, lcs, kind and flag, mism
BUBBLE_SUBST, BUBBLE_INDEL, BUBBLE_COMPLEX = 0, 1, 2   # KMC_BUBBLE_*: a record's kind, bits 0-1 of word 6
BUBBLE_REVERSED = 4       # KMC_BUBBLE_REVERSED: bit 2 of word 6, the major arm is spelled the other way round
MAP_WORDS = 8        # KMC_MAP_WORDS: reads, valid windows, placed windows, segments, crossings, fully placed reads, unplaced reads, most segments
MAP_READ_WORDS = 4   # KMC_MAP_READ_WORDS: a read's valid windows, placed windows, segments, crossings
MAP_NONE = 0xFFFFFFFF  # KMC_MAP_NONE: the low half of the place word of a window that is not placed
TRANSIT_WORDS = 8       # KMC_TRANSIT_WORDS: crossings, those without a record, unsupported records, transits stored / dropped, repeats, resolved, ambiguous
TRANSIT_PLAIN, TRANSIT_UNSPANNED, TRANSIT_RESOLVED, TRANSIT_AMBIGUOUS = 0, 1, 2, 3   # KMC_TRANSIT_*: a unitig's verdict
TRANSIT_VERDICT_NAMES = ("plain", "unspanned", "resolved", "ambiguous")
TRANSIT_ACCUMULATE = 1  # KMC_TRANSIT_ACCUMULATE: flags bit 0, add onto the result the ctx holds
CONTIG_WORDS = 8        # KMC_CONTIG_WORDS: contigs, nodes, unitigs duplicated, records ignored for support, circular, one-node, most nodes in one, bases
CONTIG_CIRCULAR = 1     # bit 0 of a contig's flags byte
PAIR_WORDS = 8          # KMC_PAIR_WORDS: pairs, UNPLACED, SPAN, PROPER, EVERTED, SAME_STRAND, records, the sum of the PROPER pairs' insert sizes
PAIR_UNPLACED, PAIR_SPAN, PAIR_PROPER, PAIR_EVERTED, PAIR_SAME_STRAND = 0, 1, 2, 3, 4   # KMC_PAIR_*: a pair's class byte
PAIR_CLASS_NAMES = ("unplaced", "span", "proper", "everted", "same_strand")
PAIR_ACCUMULATE = 1     # KMC_PAIR_ACCUMULATE: flags bit 0, add onto the result the ctx holds
CORRECT_WORDS = 8       # KMC_CORRECT_WORDS: reads, valid windows, weak windows, weak runs, candidates, corrected, ambiguous, weak windows left
CORRECT_READ_WORDS = 4  # KMC_CORRECT_READ_WORDS: a read's valid windows, weak windows, candidates, corrected
CORRECT_INTERIOR, CORRECT_HEAD, CORRECT_TAIL = 0, 1, 2   # KMC_CORRECT_*: a candidate's kind
TRIM_WORDS = 8       # KMC_TRIM_WORDS: reads, valid windows, strong windows, reads passing, reads emitted, bases emitted, emitted reads cut, their bases before
TRIM_READ_WORDS = 4  # KMC_TRIM_READ_WORDS: a read's valid windows, strong windows, span start, span length
TRIM_NONE, TRIM_ENDS, TRIM_LONGEST = 0, 1, 2   # KMC_TRIM_*: the mode
TRIM_INVERT, TRIM_PAIR_BOTH, TRIM_PAIR_EITHER = 1, 2, 4   # KMC_TRIM_*: the flag bits
TRIM_PASS, TRIM_EMITTED = 1, 2   # KMC_TRIM_*: the bits of a read's verdict byte
TRIM_MODE_NAMES = {"none": TRIM_NONE, "ends": TRIM_ENDS, "longest": TRIM_LONGEST}
NORMALIZE_WORDS = 8       # KMC_NORMALIZE_WORDS: reads, valid windows, reads emitted, bases emitted, LOW reads, DEEP reads, DEEP reads kept, sum of the depths
NORMALIZE_READ_WORDS = 4  # KMC_NORMALIZE_READ_WORDS: a read's valid windows, its own depth, its unit's depth, its unit's draw
NORM_PAIRED, NORM_INVERT = 1, 2   # KMC_NORM_*: the flag bits
NORM_KEEP, NORM_EMITTED, NORM_LOW, NORM_DEEP = 1, 2, 4, 8   # KMC_NORM_*: the bits of a read's verdict byte
SETOP_INTERSECT, SETOP_UNION, SETOP_SUBTRACT = 0, 1, 2
COUNT_LEFT, COUNT_RIGHT, COUNT_MIN, COUNT_MAX, COUNT_SUM, COUNT_DIFF = 0, 1, 2, 3, 4, 5
SETOP_NAMES = {"intersect": SETOP_INTERSECT, "union": SETOP_UNION, "subtract": SETOP_SUBTRACT}
COUNT_NAMES = {"left": COUNT_LEFT, "right": COUNT_RIGHT, "min": COUNT_MIN, "max": COUNT_MAX, "sum": COUNT_SUM, "diff": COUNT_DIFF}

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libkmc.so and the CLI tools for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", _HERE, "all"], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode:
        raise RuntimeError("building libkmc.so failed")
    return LIB_PATH


def lib() -> C.CDLL:
    """The loaded libkmc.so.  Raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `make -C {_HERE}` (or __graft_entry__.build()); "
                          "there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64/libhsa with the
    # same SONAMEs as /opt/rocm.  Importing torch first makes libkmc.so bind to the runtime torch
    # uses, so device pointers of torch tensors are valid inside libkmc (and torch still sees the
    # GPU); loading libkmc first would pin the system runtime and torch then finds no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    pu64 = C.POINTER(C.c_uint64)
    L.kmc_version.restype = C.c_char_p
    L.kmc_status_string.restype = C.c_char_p
    L.kmc_status_string.argtypes = [i32]
    L.kmc_create.argtypes = [C.POINTER(vp), C.POINTER(_Config)]
    L.kmc_destroy.argtypes = [vp]
    L.kmc_destroy.restype = None
    L.kmc_last_error.argtypes = [vp]
    L.kmc_last_error.restype = C.c_char_p
    L.kmc_reset.argtypes = [vp]
    L.kmc_add_batch.argtypes = [vp, vp, vp, u64]
    L.kmc_add_batch_device.argtypes = [vp, vp, vp, u64, u64, u64]
    L.kmc_merge_pairs_device.argtypes = [vp, vp, vp, vp, u64]
    L.kmc_finalize.argtypes = [vp, pu64, pu64]
    L.kmc_export.argtypes = [vp, vp, vp, vp, u64]
    L.kmc_export_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pu64]
    L.kmc_partition_device.argtypes = [vp, u32, pu64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.kmc_histogram.argtypes = [vp, u64, u64, u32, vp, pu64]
    L.kmc_filter_device.argtypes = [vp, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pu64, pu64]
    L.kmc_export_filtered.argtypes = [vp, u64, u64, vp, vp, vp, u64, pu64]
    L.kmc_encode_key.argtypes = [C.c_char_p, i32, i32, pu64, pu64]
    L.kmc_query.argtypes = [vp, vp, vp, u64, vp]
    L.kmc_query_device.argtypes = [vp, vp, vp, u64, vp]
    L.kmc_profile.argtypes = [vp, vp, vp, u64, u64, vp, vp]
    L.kmc_profile_device.argtypes = [vp, vp, vp, u64, u64, u64, vp, vp]
    L.kmc_compare.argtypes = [vp, vp, u64, u64, u64, u64, vp]
    L.kmc_setop_device.argtypes = [vp, vp, i32, i32, u64, u64, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pu64, pu64, vp]
    L.kmc_export_setop.argtypes = [vp, vp, i32, i32, u64, u64, u64, u64, vp, vp, vp, u64, pu64]
    L.kmc_graph_device.argtypes = [vp, u64, u64, C.POINTER(vp), pu64, vp]
    L.kmc_graph.argtypes = [vp, u64, u64, vp, u64, pu64, vp]
    L.kmc_unitigs_device.argtypes = [vp, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pu64, pu64, vp]
    L.kmc_unitigs.argtypes = [vp, u64, u64, vp, u64, vp, vp, vp, u64, pu64, pu64, vp]
    L.kmc_unitig_links_device.argtypes = [vp, u64, u64, C.POINTER(vp), C.POINTER(vp), pu64, pu64, vp]
    L.kmc_unitig_links.argtypes = [vp, u64, u64, vp, u64, vp, u64, pu64, pu64, vp]
    L.kmc_unitig_clean_device.argtypes = [vp, u64, u64, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pu64, pu64, vp]
    L.kmc_unitig_clean.argtypes = [vp, u64, u64, u64, u64, vp, vp, vp, u64, vp, u64, pu64, pu64, vp]
    L.kmc_unitig_clean_into.argtypes = [vp, vp, u64, u64, u64, u64, vp]
    L.kmc_unitig_simplify_device.argtypes = [vp, u64, u64, u64, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), pu64, pu64, vp]
    L.kmc_unitig_simplify.argtypes = [vp, u64, u64, u64, u64, u64, vp, vp, vp, u64, vp, u64, pu64, pu64, vp]
    L.kmc_unitig_simplify_into.argtypes = [vp, vp, u64, u64, u64, u64, u64, vp]
    L.kmc_unitig_components_device.argtypes = [vp, u64, u64, u64] + [C.POINTER(vp)] * 6 + [pu64, pu64, pu64, vp]
    L.kmc_unitig_components.argtypes = [vp, u64, u64, u64, vp, vp, u64, vp, u64, vp, vp, vp, u64, pu64, pu64, pu64, vp]
    L.kmc_unitig_components_into.argtypes = [vp, vp, u64, u64, u64, vp]
    # (an A/B library named by KMC_LIB_PATH may be a build from before these two: they stay unbound there and a call raises)
    if "KMC_LIB_PATH" not in os.environ or hasattr(L, "kmc_unitig_bubbles"):
        L.kmc_unitig_bubbles_device.argtypes = [vp, u64, u64, u64, C.POINTER(vp), pu64, pu64, vp]
        L.kmc_unitig_bubbles.argtypes = [vp, u64, u64, u64, vp, u64, pu64, pu64, vp]
    L.kmc_unitig_map_device.argtypes = [vp, u64, u64, vp, vp, u64, u64] + [C.POINTER(vp)] * 5 + [pu64, pu64, vp]
    L.kmc_unitig_map.argtypes = [vp, u64, u64, vp, vp, u64, vp, vp, vp, vp, u64, vp, u64, pu64, pu64, vp]
    if "KMC_LIB_PATH" not in os.environ or hasattr(L, "kmc_unitig_transits"):   # (as for the bubbles calls above)
        L.kmc_unitig_transits_device.argtypes = [vp, u64, u64, u64, u32, vp, vp, u64, u64] + [C.POINTER(vp)] * 4 + [pu64, pu64, pu64, vp]
        L.kmc_unitig_transits.argtypes = [vp, u64, u64, u64, u32, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, pu64, pu64, pu64, vp]
    if "KMC_LIB_PATH" not in os.environ or hasattr(L, "kmc_unitig_contigs"):   # (as for the bubbles calls above)
        L.kmc_unitig_contigs_device.argtypes = [vp, u64, u64, u64, u64] + [C.POINTER(vp)] * 6 + [pu64, pu64, pu64, vp]
        L.kmc_unitig_contigs.argtypes = [vp, u64, u64, u64, u64, vp, u64, vp, vp, vp, vp, u64, vp, u64, pu64, pu64, pu64, vp]
    if "KMC_LIB_PATH" not in os.environ or hasattr(L, "kmc_unitig_pairs"):   # (as for the bubbles calls above)
        L.kmc_unitig_pairs_device.argtypes = [vp, u64, u64, u64, u32, vp, vp, u64, u64] + [C.POINTER(vp)] * 9 + [pu64, pu64, vp]
        L.kmc_unitig_pairs.argtypes = [vp, u64, u64, u64, u32, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp, u64, pu64, pu64, vp]
    L.kmc_correct_device.argtypes = [vp, u64, u64, vp, vp, u64, u64] + [C.POINTER(vp)] * 4 + [pu64, vp]
    L.kmc_correct.argtypes = [vp, u64, u64, vp, vp, u64, vp, vp, vp, vp, u64, pu64, vp]
    L.kmc_trim_device.argtypes = [vp, u64, u64, i32, u32, u64, u32, u64, vp, vp, u64, u64] + [C.POINTER(vp)] * 5 + [pu64, pu64, vp]
    L.kmc_trim.argtypes = [vp, u64, u64, i32, u32, u64, u32, u64, vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, pu64, pu64, vp]
    if "KMC_LIB_PATH" not in os.environ or hasattr(L, "kmc_normalize"):   # (as for the bubbles calls above)
        L.kmc_normalize_device.argtypes = [vp, u32, u64, u64, u64, u32, vp, vp, u64, u64] + [C.POINTER(vp)] * 5 + [pu64, pu64, vp]
        L.kmc_normalize.argtypes = [vp, u32, u64, u64, u64, u32, vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, pu64, pu64, vp]
    L.kmc_owner_of.argtypes = [u64, u64, u32]
    L.kmc_owner_of.restype = u32
    L.kmc_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.kmc_slab_words.argtypes = [vp, u64]
    L.kmc_slab_words.restype = u64
    L.kmc_pack_slab_device.argtypes = [vp, vp, u64]
    L.kmc_merge_slabs_device.argtypes = [vp, vp, u32, u64, u32, u32]
    L.kmc_forget_source.argtypes = [vp, i32]
    L.kmc_poll.argtypes = [vp]
    L.kmc_sync.argtypes = [vp]
    L.kmc_finalize_async.argtypes = [vp]
    L.kmc_read_peak_device.argtypes = [vp, u64, i32, vp, i32, i32, C.POINTER(C.c_double), pu64]
    L.kmc_read_pieces.argtypes = [u64, i32, vp, vp, u64]
    L.kmc_read_pieces.restype = u64
    L.kmc_count_file.argtypes = [vp, C.c_char_p, pu64, pu64]
    L.kmc_count_file_multi.argtypes = [C.POINTER(vp), u32, C.c_char_p, pu64, pu64]
    L.kmc_parse_fasta.argtypes = [C.c_char_p, C.POINTER(_Reads), C.c_char_p, C.c_size_t]
    L.kmc_free_reads.argtypes = [C.POINTER(_Reads)]
    L.kmc_free_reads.restype = None
    L.kmc_fasta_stream_open.argtypes = [C.c_char_p, u64, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.kmc_fasta_stream_next.argtypes = [vp, C.POINTER(_Reads), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.kmc_fasta_stream_close.argtypes = [vp]
    L.kmc_fasta_stream_close.restype = None
    L.kmc_decode_key.argtypes = [u64, u64, i32, C.c_char_p]
    L.kmc_decode_key.restype = None
    L.kmc_synth_records_for_bytes.argtypes = [C.POINTER(Synth), u64, pu64]
    L.kmc_synth_records_for_bytes.restype = u64
    L.kmc_synth_reads_host.argtypes = [C.POINTER(Synth), u64, u64, vp, vp]
    L.kmc_synth_reads_device.argtypes = [C.POINTER(Synth), u64, u64, vp, vp, i32, vp]
    L.kmc_synth_write_fasta.argtypes = [C.POINTER(Synth), u64, u64, vp]
    _lib = L
    return L


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------
_CODE = np.frombuffer(b"ACGT", dtype=np.uint8)


@dataclass
class Table:
    """Sorted count table: ascending by (key_hi, key_lo) == string order (main.rs:87)."""
    key_hi: np.ndarray
    key_lo: np.ndarray
    count: np.ndarray
    klen: int

    @property
    def n_distinct(self) -> int:
        return int(self.key_lo.shape[0])

    @property
    def n_total(self) -> int:
        return int(self.count.sum(dtype=np.uint64)) if self.n_distinct else 0

    def kmers(self) -> np.ndarray:
        """(n_distinct, klen) uint8 ASCII matrix."""
        n, k = self.n_distinct, self.klen
        out = np.empty((n, k), dtype=np.uint8)
        lo = self.key_lo.astype(np.uint64).copy()
        hi = self.key_hi.astype(np.uint64).copy()
        for i in range(k - 1, -1, -1):
            out[:, i] = _CODE[(lo & np.uint64(3)).astype(np.intp)]
            lo = (lo >> np.uint64(2)) | (hi << np.uint64(62))
            hi = hi >> np.uint64(2)
        return out

    def to_bytes(self, expand: bool = False) -> bytes:
        """``KMER\\tCOUNT\\n`` lines, or with expand=True every key repeated COUNT times, one per
        line: byte-identical to the reference's output loop, main.rs:88-90."""
        n, k = self.n_distinct, self.klen
        if n == 0:
            return b""
        km = self.kmers()
        if expand:
            lines = np.empty((n, k + 1), dtype=np.uint8)
            lines[:, :k] = km
            lines[:, k] = 10
            return np.repeat(lines, self.count.astype(np.intp), axis=0).tobytes()
        parts = []
        for i in range(n):
            parts.append(km[i].tobytes() + b"\t%d\n" % int(self.count[i]))
        return b"".join(parts)

    def digest(self, expand: bool = False) -> str:
        """sha256 of to_bytes(), computed in slices (the expanded LR output is ~195 MB)."""
        h = hashlib.sha256()
        n = self.n_distinct
        step = 1 << 16
        for s in range(0, n, step):
            h.update(Table(self.key_hi[s:s + step], self.key_lo[s:s + step], self.count[s:s + step], self.klen).to_bytes(expand))
        return h.hexdigest()

    def equals(self, other: "Table") -> bool:
        return (self.klen == other.klen and self.n_distinct == other.n_distinct
                and np.array_equal(self.key_hi, other.key_hi) and np.array_equal(self.key_lo, other.key_lo)
                and np.array_equal(self.count, other.count))


_COMPARE_FIELDS = ("n_a", "n_b", "n_both", "sum_a", "sum_b", "shared_sum_a", "shared_sum_b", "sum_min")


@dataclass
class Comparison:
    """The eight words of kmc_compare and the similarities that are host arithmetic on them (0.0 where a
    denominator is 0: two empty sides are not similar, and not NaN)."""
    n_a: int
    n_b: int
    n_both: int
    sum_a: int
    sum_b: int
    shared_sum_a: int
    shared_sum_b: int
    sum_min: int

    @classmethod
    def from_words(cls, words) -> "Comparison":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _COMPARE_FIELDS]

    @staticmethod
    def _ratio(num: int, den: int) -> float:
        return num / den if den else 0.0

    @property
    def union(self) -> int:
        return self.n_a + self.n_b - self.n_both

    @property
    def jaccard(self) -> float:
        return self._ratio(self.n_both, self.union)

    @property
    def containment_a(self) -> float:
        return self._ratio(self.n_both, self.n_a)

    @property
    def containment_b(self) -> float:
        return self._ratio(self.n_both, self.n_b)

    @property
    def weighted_jaccard(self) -> float:
        return self._ratio(self.sum_min, self.sum_a + self.sum_b - self.sum_min)

    @property
    def bray_curtis(self) -> float:
        """Bray-Curtis similarity 2 sum(min) / (sum_a + sum_b)."""
        return self._ratio(2 * self.sum_min, self.sum_a + self.sum_b)

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines as the CLI's --compare prints them."""
        lines = ["%s\t%d" % (f, getattr(self, f)) for f in _COMPARE_FIELDS]
        lines.append("union\t%d" % self.union)
        for f in ("jaccard", "containment_a", "containment_b", "weighted_jaccard", "bray_curtis"):
            lines.append("%s\t%.6f" % (f, getattr(self, f)))
        return "\n".join(lines) + "\n"


_GRAPH_FIELDS = ("nodes", "right_degrees", "left_degrees", "isolated", "dead_ends", "branching", "end_sides", "single_node_unitigs")


@dataclass
class GraphSummary:
    """The eight words of kmc_graph over the solid keys: nodes, the sums of the right and left degrees, nodes without a
    neighbour, nodes with neighbours on one side only, nodes with a degree of 2 or more, sides that end a unitig, nodes
    that are a unitig of their own."""
    nodes: int
    right_degrees: int
    left_degrees: int
    isolated: int
    dead_ends: int
    branching: int
    end_sides: int
    single_node_unitigs: int

    @classmethod
    def from_words(cls, words) -> "GraphSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _GRAPH_FIELDS]

    @property
    def unitigs(self) -> int:
        """Non-circular unitigs: every one has two end sides."""
        return self.end_sides // 2

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines as the CLI's --graph-stats prints them."""
        lines = ["%s\t%d" % (f, getattr(self, f)) for f in _GRAPH_FIELDS]
        lines.append("unitigs\t%d" % self.unitigs)
        return "\n".join(lines) + "\n"


_UNITIG_FIELDS = ("unitigs", "bases", "keys", "circular", "one_key", "longest_keys", "unjoined_sides", "abundance")


@dataclass
class UnitigSummary:
    """The eight words of kmc_unitigs over the solid keys: unitigs, their bases, their keys (= the solid keys), circular
    unitigs, unitigs of one key, the keys of the longest unitig, sides that continue in the graph but are not joined
    (hairpins, palindromes), the sum of all abundances."""
    unitigs: int
    bases: int
    keys: int
    circular: int
    one_key: int
    longest_keys: int
    unjoined_sides: int
    abundance: int

    @classmethod
    def from_words(cls, words) -> "UnitigSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _UNITIG_FIELDS]

    @property
    def mean_keys(self) -> float:
        """Keys per unitig."""
        return self.keys / self.unitigs if self.unitigs else 0.0

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _UNITIG_FIELDS) + "\n"


@dataclass
class Unitigs:
    """What KmerCounter.unitigs returns: ``bases`` uint8[n_bases] (ASCII, concatenated), ``offsets`` uint64[n + 1], ``abund``
    uint64[n] (summed counts of a unitig's keys), ``flags`` uint8[n] (UNITIG_CIRCULAR), ``summary``."""
    bases: np.ndarray
    offsets: np.ndarray
    abund: np.ndarray
    flags: np.ndarray
    summary: UnitigSummary

    def __len__(self) -> int:
        return len(self.abund)

    def strings(self) -> list:
        text = self.bases.tobytes().decode("ascii")
        o = self.offsets
        return [text[int(o[i]):int(o[i + 1])] for i in range(len(self))]

    def to_fasta(self) -> str:
        """FASTA as the CLI's --unitigs prints it: ``>INDEX LN:i:BASES KC:i:ABUND CL:i:0|1`` and the sequence on one line."""
        return "".join(">%d LN:i:%d KC:i:%d CL:i:%d\n%s\n" % (i, len(s), int(self.abund[i]), int(self.flags[i]) & UNITIG_CIRCULAR, s)
                       for i, s in enumerate(self.strings()))

    def to_gfa(self, links: "UnitigLinks", k: int, transits: Optional["Transits"] = None, contigs: Optional["Contigs"] = None) -> str:
        """GFA 1.0 as the CLI's --gfa prints it: ``H VN:Z:1.0``, one ``S INDEX SEQ LN:i:BASES KC:i:ABUND CL:i:0|1`` per
        unitig, one ``L U +|- V +|- (k-1)M`` per record of ``links`` (KmerCounter.unitig_links of the same range), tab-separated.
        With ``transits`` (KmerCounter.transits of the same range) every ``L`` line ends in ``RC:i:SUPPORT``, the reads that
        walked the link.  With ``contigs`` (KmerCounter.contigs of the same range) one ``P INDEX U+,V-,... OVERLAPS`` line per
        contig follows: its unitig path, ``(k-1)M`` between neighbours, and once more at the end of a circular one."""
        if len(links.offsets) != 2 * len(self) + 1:
            raise ValueError("the links are not those of these unitigs")
        if transits is not None and len(transits.link_support) != len(links):
            raise ValueError("the transits are not those of these links")
        out = ["H\tVN:Z:1.0\n"]
        out += ["S\t%d\t%s\tLN:i:%d\tKC:i:%d\tCL:i:%d\n" % (i, s, len(s), int(self.abund[i]), int(self.flags[i]) & UNITIG_CIRCULAR)
                for i, s in enumerate(self.strings())]
        if transits is None:
            out += ["L\t%d\t%s\t%d\t%s\t%dM\n" % (u, o1, v, o2, k - 1) for u, o1, v, o2 in links.records()]
        else:
            out += ["L\t%d\t%s\t%d\t%s\t%dM\tRC:i:%d\n" % (u, o1, v, o2, k - 1, int(n))
                    for (u, o1, v, o2), n in zip(links.records(), transits.link_support)]
        if contigs is not None:
            if len(contigs.path) and int(contigs.path.max()) >> 1 >= len(self):
                raise ValueError("the contigs are not those of these unitigs")
            for i, (p, f) in enumerate(zip(contigs.paths(), contigs.flags)):
                n_overlaps = len(p) - 1 + (int(f) & CONTIG_CIRCULAR)
                out.append("P\t%d\t%s\t%s\n" % (i, ",".join("%d%s" % (e >> 1, "-" if e & 1 else "+") for e in p),
                                                 ",".join(["%dM" % (k - 1)] * n_overlaps) or "*"))
        return "".join(out)


_LINK_FIELDS = ("unitigs", "records", "ends_without", "ends_branching", "self_records", "dropped", "isolated_unitigs", "max_records")


@dataclass
class LinkSummary:
    """The eight words of kmc_unitig_links: unitigs, link records, unitig ends with no record, ends with two or more,
    records whose target is the source's own unitig, extensions dropped because the side they reach is not a terminal
    (around palindromic keys), unitigs with no record at either end, the most records at one end."""
    unitigs: int
    records: int
    ends_without: int
    ends_branching: int
    self_records: int
    dropped: int
    isolated_unitigs: int
    max_records: int

    @classmethod
    def from_words(cls, words) -> "LinkSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _LINK_FIELDS]

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _LINK_FIELDS) + "\n"


@dataclass
class UnitigLinks:
    """What KmerCounter.unitig_links returns: ``offsets`` uint64[2 n + 1] indexed by unitig end (2u: the START end of unitig
    u, 2u + 1: its END end), ``to`` uint32[records] (the target ends), ``summary``.  The records of end i are
    ``to[offsets[i]:offsets[i + 1]]``."""
    offsets: np.ndarray
    to: np.ndarray
    summary: LinkSummary

    def __len__(self) -> int:
        return len(self.to)

    def records(self):
        """(u, o1, v, o2) per record in array order, in GFA terms: leaving u through its END end reads ``u +``, through
        its START end ``u -``; arriving at the START end of v reads ``v +``, at its END end ``v -``."""
        o = self.offsets
        for i in range(len(o) - 1):
            for t in self.to[int(o[i]):int(o[i + 1])]:
                yield i >> 1, "+" if i & 1 else "-", int(t) >> 1, "-" if int(t) & 1 else "+"


_MAP_FIELDS = ("reads", "valid_windows", "placed_windows", "segments", "crossings", "reads_fully_placed", "reads_unplaced", "max_segments")


@dataclass
class MapSummary:
    """The eight words of kmc_unitig_map: reads, valid windows, placed windows, segments, crossings, reads with at least one
    valid window and all of them placed, reads with no placed window, the most segments in one read."""
    reads: int
    valid_windows: int
    placed_windows: int
    segments: int
    crossings: int
    reads_fully_placed: int
    reads_unplaced: int
    max_segments: int

    @classmethod
    def from_words(cls, words) -> "MapSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _MAP_FIELDS]

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _MAP_FIELDS) + "\n"


@dataclass
class ReadMap:
    """What KmerCounter.map_reads returns: ``place`` uint64[n_bases] (low half 2 * unitig + orientation or MAP_NONE, high
    half the key position), ``stats`` uint32[n_reads, 4], ``seg_offsets`` uint64[n_reads + 1], ``segments`` uint32[n, 4]
    (start, len, 2 * unitig + orientation, pos), ``support`` uint64[n_unitigs], ``summary``.  The segments of read r are
    ``segments[seg_offsets[r]:seg_offsets[r + 1]]``."""
    place: np.ndarray
    stats: np.ndarray
    seg_offsets: np.ndarray
    segments: np.ndarray
    support: np.ndarray
    summary: MapSummary

    def __len__(self) -> int:
        return len(self.seg_offsets) - 1

    def walks(self) -> list:
        """Per read a list of stretches; a stretch is a list of ``(unitig, orientation, pos, len)`` in which each element is
        a crossing of the one before it (it starts at the window right behind it), and a gap starts a new stretch."""
        out = []
        so = self.seg_offsets
        for r in range(len(self)):
            stretches, end = [], None
            for start, ln, uni, pos in self.segments[int(so[r]):int(so[r + 1])].tolist():
                if end is None or start != end:
                    stretches.append([])
                stretches[-1].append((uni >> 1, uni & 1, pos, ln))
                end = start + ln
            out.append(stretches)
        return out

    def walk_text(self, r: int) -> str:
        """The WALK column of ``k-mer-count --map`` for read r: ``>U:POS:LEN`` / ``<U:POS:LEN`` per segment, a crossing written
        directly behind its predecessor, ``,`` at a gap, ``*`` for a read without a segment."""
        so = self.seg_offsets
        parts, end = [], None
        for start, ln, uni, pos in self.segments[int(so[r]):int(so[r + 1])].tolist():
            if end is not None and start != end:
                parts.append(",")
            parts.append("%s%d:%d:%d" % ("<" if uni & 1 else ">", uni >> 1, pos, ln))
            end = start + ln
        return "".join(parts) or "*"


_TRANSIT_FIELDS = ("crossings", "crossings_without_record", "records_unsupported", "transits", "transits_dropped", "repeats", "resolved", "ambiguous")


@dataclass
class TransitSummary:
    """The eight words of kmc_unitig_transits: crossings, crossings with no link record in either direction, records with
    support 0, transits stored, transits dropped for a missing record, repeat unitigs, RESOLVED ones, AMBIGUOUS ones."""
    crossings: int
    crossings_without_record: int
    records_unsupported: int
    transits: int
    transits_dropped: int
    repeats: int
    resolved: int
    ambiguous: int

    @classmethod
    def from_words(cls, words) -> "TransitSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _TRANSIT_FIELDS]

    @property
    def unspanned(self) -> int:
        return self.repeats - self.resolved - self.ambiguous

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _TRANSIT_FIELDS) + "\n"


@dataclass
class Transits:
    """What KmerCounter.transits returns: ``link_support`` uint64[records] indexed like ``links.to``, ``transit_offsets``
    uint64[n_unitigs + 1], ``transit_count`` uint64[slots] (unitig u: a dS x dE matrix, row P a record rank at its START
    end, column Q one at its END end), ``verdict`` uint8[n_unitigs] (TRANSIT_PLAIN / UNSPANNED / RESOLVED / AMBIGUOUS),
    ``summary``, and ``links``, the UnitigLinks they are indexed by."""
    link_support: np.ndarray
    transit_offsets: np.ndarray
    transit_count: np.ndarray
    verdict: np.ndarray
    summary: TransitSummary
    links: UnitigLinks

    def __len__(self) -> int:
        return len(self.verdict)

    def degrees(self, u: int) -> Tuple[int, int]:
        """(dS, dE): the records at the START and at the END end of unitig u"""
        o = self.links.offsets
        return int(o[2 * u + 1]) - int(o[2 * u]), int(o[2 * u + 2]) - int(o[2 * u + 1])

    def matrix(self, u: int) -> np.ndarray:
        """The dS x dE transit counts of unitig u (an array without entries if one of its ends is bare)."""
        ds, de = self.degrees(u)
        return self.transit_count[int(self.transit_offsets[u]):int(self.transit_offsets[u + 1])].reshape(ds, de)

    def records(self):
        """(end, to, support) per link record, in array order."""
        o = self.links.offsets
        for e in range(len(o) - 1):
            for j in range(int(o[e]), int(o[e + 1])):
                yield e, int(self.links.to[j]), int(self.link_support[j])

    def to_text(self) -> str:
        """What ``k-mer-count --transits`` prints: ``L END TO SUPPORT`` per record with support, then per repeat unitig
        ``U UNITIG VERDICT DS DE`` and its non-zero slots ``T UNITIG P Q COUNT``, tab-separated, in array order."""
        out = ["L\t%d\t%d\t%d\n" % r for r in self.records() if r[2]]
        for u in np.flatnonzero(self.verdict != TRANSIT_PLAIN).tolist():
            m = self.matrix(u)
            out.append("U\t%d\t%s\t%d\t%d\n" % (u, TRANSIT_VERDICT_NAMES[int(self.verdict[u])], m.shape[0], m.shape[1]))
            out += ["T\t%d\t%d\t%d\t%d\n" % (u, p, q, int(m[p, q])) for p in range(m.shape[0]) for q in range(m.shape[1]) if m[p, q]]
        return "".join(out)


_PAIR_FIELDS = ("pairs", "unplaced", "span", "proper", "everted", "same_strand", "records", "insert_sum")


@dataclass
class PairSummary:
    """The eight words of kmc_unitig_pairs: pairs, then those UNPLACED, SPAN, PROPER, EVERTED and SAME_STRAND, the pair
    records, and the sum of the insert sizes of the PROPER pairs."""
    pairs: int
    unplaced: int
    span: int
    proper: int
    everted: int
    same_strand: int
    records: int
    insert_sum: int

    @classmethod
    def from_words(cls, words) -> "PairSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _PAIR_FIELDS]

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _PAIR_FIELDS) + "\n"


@dataclass
class PairLinks:
    """What KmerCounter.pair_links returns.  Per pair of the batch: ``pair_class`` uint8[n_pairs] (PAIR_*), ``pair_ends``
    uint32[n_pairs, 2] (the out ends of mates A and B, MAP_NONE without an anchor), ``pair_value`` uint64[n_pairs] (R for a
    SPAN pair, the insert size F for a PROPER one, else 0).  Per record, in ascending (a, b): ``rec_ends`` uint32[records, 2],
    ``rec_count``, ``rec_sum``, ``rec_min``, ``rec_max`` uint64[records] over R of the SPAN pairs between those two ends.
    ``insert_hist`` uint64[n_bins]: PROPER pairs per insert size, the last bin open.  With ``accumulate`` the records, the
    histogram and the summary are totals over the batches so far."""
    pair_class: np.ndarray
    pair_ends: np.ndarray
    pair_value: np.ndarray
    rec_ends: np.ndarray
    rec_count: np.ndarray
    rec_sum: np.ndarray
    rec_min: np.ndarray
    rec_max: np.ndarray
    insert_hist: np.ndarray
    summary: PairSummary

    def __len__(self) -> int:
        return len(self.rec_count)

    def records(self):
        """(a, b, count, sum, min, max) per record, in array order."""
        for (a, b), c, s, lo, hi in zip(self.rec_ends.tolist(), self.rec_count.tolist(), self.rec_sum.tolist(), self.rec_min.tolist(),
                                        self.rec_max.tolist()):
            yield a, b, c, s, lo, hi

    def insert_median(self) -> Optional[int]:
        """The lower median of the insert sizes in ``insert_hist`` (None without a PROPER pair; the open last bin counts as
        its index)."""
        total = int(self.insert_hist.sum())
        if not total:
            return None
        return int(np.searchsorted(np.cumsum(self.insert_hist), (total + 1) // 2))

    def gaps(self, insert: float) -> np.ndarray:
        """float64[records]: the estimated bases between the two ends of every record under a library insert size,
        ``insert - sum / count``; -(k - 1) where the two ends are joined by a link."""
        return float(insert) - self.rec_sum.astype(np.float64) / self.rec_count.astype(np.float64)

    def to_text(self) -> str:
        """What ``k-mer-count --pairs`` prints: ``I F PAIRS`` per non-zero bin of the insert histogram, then ``P A B COUNT SUM
        MIN MAX`` per record, tab-separated."""
        out = ["I\t%d\t%d\n" % (f, int(self.insert_hist[f])) for f in np.flatnonzero(self.insert_hist).tolist()]
        out += ["P\t%d\t%d\t%d\t%d\t%d\t%d\n" % r for r in self.records()]
        return "".join(out)


_CONTIG_FIELDS = ("contigs", "nodes", "unitigs_duplicated", "records_ignored", "circular", "one_node", "most_nodes", "bases")


@dataclass
class ContigSummary:
    """The eight words of kmc_unitig_contigs: contigs, nodes (path entries), unitigs duplicated, link records ignored for
    support at the ends of single-copy unitigs, circular contigs, contigs of one node, the most nodes in one contig, bases."""
    contigs: int
    nodes: int
    unitigs_duplicated: int
    records_ignored: int
    circular: int
    one_node: int
    most_nodes: int
    bases: int

    @classmethod
    def from_words(cls, words) -> "ContigSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _CONTIG_FIELDS]

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _CONTIG_FIELDS) + "\n"


@dataclass
class Contigs:
    """What KmerCounter.contigs returns: ``bases`` uint8[n_bases] (ASCII, concatenated), ``offsets`` uint64[n + 1],
    ``path_offsets`` uint64[n + 1], ``path`` uint32[n_nodes] (entries 2 * unitig + o, o = 1: read reverse-complemented),
    ``abund`` uint64[n] (the unitigs' abundances summed over the path; a duplicated repeat counts in full in each copy),
    ``flags`` uint8[n] (CONTIG_CIRCULAR), ``summary``."""
    bases: np.ndarray
    offsets: np.ndarray
    path_offsets: np.ndarray
    path: np.ndarray
    abund: np.ndarray
    flags: np.ndarray
    summary: ContigSummary

    def __len__(self) -> int:
        return len(self.abund)

    def strings(self) -> list:
        text = self.bases.tobytes().decode("ascii")
        o = self.offsets
        return [text[int(o[i]):int(o[i + 1])] for i in range(len(self))]

    def paths(self) -> list:
        """per contig the list of its path entries 2 * unitig + o"""
        o = self.path_offsets
        return [self.path[int(o[i]):int(o[i + 1])].tolist() for i in range(len(self))]

    def walks(self) -> list:
        """per contig its path as ReadMap.walks() writes one: ``>U`` / ``<U`` per unitig, concatenated"""
        return ["".join("%s%d" % ("<" if e & 1 else ">", e >> 1) for e in p) for p in self.paths()]

    def to_fasta(self) -> str:
        """FASTA as the CLI's --contigs prints it: ``>INDEX LN:i:BASES KC:i:ABUND CL:i:0|1 WK:Z:WALK`` and the sequence on one line."""
        return "".join(">%d LN:i:%d KC:i:%d CL:i:%d WK:Z:%s\n%s\n" % (i, len(s), int(self.abund[i]), int(self.flags[i]) & CONTIG_CIRCULAR, w, s)
                       for i, (s, w) in enumerate(zip(self.strings(), self.walks())))

    def to_text(self) -> str:
        """What ``k-mer-count --contigs`` prints: to_fasta()."""
        return self.to_fasta()


_CORRECT_FIELDS = ("reads", "valid_windows", "weak_windows", "weak_runs", "candidates", "corrected", "ambiguous", "weak_windows_left")


@dataclass
class CorrectSummary:
    """The eight words of kmc_correct: reads, valid windows, weak windows, weak runs, candidates, corrected candidates,
    ambiguous candidates, weak windows left behind the corrections."""
    reads: int
    valid_windows: int
    weak_windows: int
    weak_runs: int
    candidates: int
    corrected: int
    ambiguous: int
    weak_windows_left: int

    @classmethod
    def from_words(cls, words) -> "CorrectSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _CORRECT_FIELDS]

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _CORRECT_FIELDS) + "\n"


@dataclass
class CorrectedReads:
    """What KmerCounter.correct_reads returns: ``bases`` uint8[n_bases] (the batch with the corrected positions replaced) and
    the caller's ``offsets``, ``stats`` uint32[n_reads, 4] (valid windows, weak windows, candidates, corrected),
    ``cand_offsets`` uint64[n_reads + 1], ``cands`` uint32[n, 4] (p, old | new << 8 | kind << 16 | accepted mask << 24, a, n),
    ``summary``.  The candidates of read r are ``cands[cand_offsets[r]:cand_offsets[r + 1]]``."""
    bases: np.ndarray
    offsets: np.ndarray
    stats: np.ndarray
    cand_offsets: np.ndarray
    cands: np.ndarray
    summary: CorrectSummary

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def strings(self) -> list:
        """The corrected reads as str."""
        o, b = self.offsets, self.bases.tobytes()
        return [b[int(o[i]):int(o[i + 1])].decode("latin-1") for i in range(len(self))]

    def fixes(self):
        """``(read, pos, old, new, kind)`` of every corrected candidate, in array order."""
        co = self.cand_offsets
        for r in range(len(self)):
            for p, word, _, _ in self.cands[int(co[r]):int(co[r + 1])].tolist():
                if (word & 255) != (word >> 8 & 255):
                    yield r, p, chr(word & 255), chr(word >> 8 & 255), word >> 16 & 255

    def to_fasta(self) -> str:
        """What ``k-mer-count --correct`` prints: ``>INDEX WINDOWS WEAK CANDIDATES FIXED`` and the corrected read."""
        return "".join(">%d %d %d %d %d\n%s\n" % (i, s[0], s[1], s[2], s[3], r) for i, (s, r) in enumerate(zip(self.stats.tolist(), self.strings())))


_TRIM_FIELDS = ("reads", "valid_windows", "strong_windows", "passed", "emitted", "bases", "cut_reads", "bases_before")


@dataclass
class TrimSummary:
    """The eight words of kmc_trim: reads, valid windows, strong windows, reads whose own PASS is true, reads emitted, bases
    emitted, emitted reads whose span is shorter than the read, the bases of the emitted reads before trimming."""
    reads: int
    valid_windows: int
    strong_windows: int
    passed: int
    emitted: int
    bases: int
    cut_reads: int
    bases_before: int

    @classmethod
    def from_words(cls, words) -> "TrimSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _TRIM_FIELDS]

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _TRIM_FIELDS) + "\n"


@dataclass
class TrimmedReads:
    """What KmerCounter.trim_reads returns: the emitted spans as a batch -- ``bases`` uint8[n_out_bases], ``offsets``
    uint64[n_out + 1] -- with ``origin`` uint64[n_out] (the source read of each), and for every read of the input ``stats``
    uint32[n_reads, 4] (valid windows, strong windows, span start, span length) and ``verdict`` uint8[n_reads] (TRIM_PASS |
    TRIM_EMITTED); ``summary``."""
    bases: np.ndarray
    offsets: np.ndarray
    origin: np.ndarray
    stats: np.ndarray
    verdict: np.ndarray
    summary: TrimSummary

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def strings(self) -> list:
        """The emitted spans as str."""
        o, b = self.offsets, self.bases.tobytes()
        return [b[int(o[i]):int(o[i + 1])].decode("latin-1") for i in range(len(self))]

    def to_fasta(self) -> str:
        """What ``k-mer-count --trim`` prints, emitted reads only: ``>INDEX WINDOWS STRONG START LEN`` and the span."""
        st = self.stats.tolist()
        return "".join(">%d %d %d %d %d\n%s\n" % ((r,) + tuple(st[r]) + (s,)) for r, s in zip(self.origin.tolist(), self.strings()))


_NORMALIZE_FIELDS = ("reads", "valid_windows", "emitted", "bases", "low", "deep", "deep_kept", "depth_sum")


@dataclass
class NormalizeSummary:
    """The eight words of kmc_normalize: reads, valid windows, reads emitted, bases emitted, LOW reads, DEEP reads, DEEP
    reads that are kept, the sum of the reads' own depths."""
    reads: int
    valid_windows: int
    emitted: int
    bases: int
    low: int
    deep: int
    deep_kept: int
    depth_sum: int

    @classmethod
    def from_words(cls, words) -> "NormalizeSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _NORMALIZE_FIELDS]

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _NORMALIZE_FIELDS) + "\n"


@dataclass
class NormalizedReads:
    """What KmerCounter.normalize_reads returns: the emitted reads as a batch -- ``bases`` uint8[n_out_bases], ``offsets``
    uint64[n_out + 1] -- with ``origin`` uint64[n_out] (the source read of each), and for every read of the input ``stats``
    uint32[n_reads, 4] (valid windows, own depth, unit depth, draw) and ``verdict`` uint8[n_reads] (NORM_KEEP | NORM_EMITTED |
    NORM_LOW | NORM_DEEP); ``summary``."""
    bases: np.ndarray
    offsets: np.ndarray
    origin: np.ndarray
    stats: np.ndarray
    verdict: np.ndarray
    summary: NormalizeSummary

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def strings(self) -> list:
        """The emitted reads as str."""
        o, b = self.offsets, self.bases.tobytes()
        return [b[int(o[i]):int(o[i + 1])].decode("latin-1") for i in range(len(self))]

    def to_fasta(self) -> str:
        """What ``k-mer-count --normalize`` prints, emitted reads only: ``>INDEX WINDOWS DEPTH UNITDEPTH`` and the read."""
        st = self.stats.tolist()
        return "".join(">%d %d %d %d\n%s\n" % ((r,) + tuple(st[r][:3]) + (s,)) for r, s in zip(self.origin.tolist(), self.strings()))


_CLEAN_FIELDS = ("unitigs", "tips", "islands", "kept_keys", "tip_keys", "island_keys", "tip_candidates", "kept_count")


@dataclass
class CleanSummary:
    """The eight words of kmc_unitig_clean: unitigs, those clipped as tips, those dropped as islands, the keys kept, the keys
    of the tips, the keys of the islands, tip candidates (those that survive included), the sum of the counts of the kept keys."""
    unitigs: int
    tips: int
    islands: int
    kept_keys: int
    tip_keys: int
    island_keys: int
    tip_candidates: int
    kept_count: int

    @classmethod
    def from_words(cls, words) -> "CleanSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _CLEAN_FIELDS]

    @property
    def removed(self) -> int:
        """Unitigs this pass takes out."""
        return self.tips + self.islands

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _CLEAN_FIELDS) + "\n"


@dataclass
class CleanedUnitigs:
    """What KmerCounter.clean_unitigs returns: ``table`` (the keys of the kept unitigs with their counts, in view order),
    ``verdict`` uint8[n unitigs] (CLEAN_KEEP / CLEAN_TIP / CLEAN_ISLAND, indexed as unitigs() numbers them), ``summary``."""
    table: "Table"
    verdict: np.ndarray
    summary: CleanSummary


_SIMPLIFY_FIELDS = _CLEAN_FIELDS + ("bubbles", "bubble_keys", "bubble_candidates", "bubble_count")


@dataclass
class SimplifySummary:
    """The twelve words of kmc_unitig_simplify: those of CleanSummary (kept_keys and kept_count after all three removals),
    then the bubbles popped, their keys, bubble candidates (those that survive included), the sum of the counts of the
    popped bubbles' keys."""
    unitigs: int
    tips: int
    islands: int
    kept_keys: int
    tip_keys: int
    island_keys: int
    tip_candidates: int
    kept_count: int
    bubbles: int
    bubble_keys: int
    bubble_candidates: int
    bubble_count: int

    @classmethod
    def from_words(cls, words) -> "SimplifySummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _SIMPLIFY_FIELDS]

    @property
    def removed(self) -> int:
        """Unitigs this pass takes out."""
        return self.tips + self.islands + self.bubbles

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _SIMPLIFY_FIELDS) + "\n"


@dataclass
class SimplifiedUnitigs:
    """What KmerCounter.simplify_unitigs returns: ``table``, ``verdict`` uint8[n unitigs] (CLEAN_KEEP / CLEAN_TIP /
    CLEAN_ISLAND / CLEAN_BUBBLE), ``summary``."""
    table: "Table"
    verdict: np.ndarray
    summary: SimplifySummary


_COMPONENT_FIELDS = ("unitigs", "components", "single_unitig", "max_keys", "max_unitigs", "small", "kept_keys", "kept_count")


@dataclass
class ComponentSummary:
    """The eight words of kmc_unitig_components: unitigs, components, components of one unitig, the most keys and the most
    unitigs in one component, small components, the keys kept, the sum of the counts of the kept keys."""
    unitigs: int
    components: int
    single_unitig: int
    max_keys: int
    max_unitigs: int
    small: int
    kept_keys: int
    kept_count: int

    @classmethod
    def from_words(cls, words) -> "ComponentSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _COMPONENT_FIELDS]

    @property
    def removed(self) -> int:
        """Components this pass takes out."""
        return self.small

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _COMPONENT_FIELDS) + "\n"


@dataclass
class Components:
    """What KmerCounter.components returns: ``comp_of`` uint32[n unitigs] (the component of each unitig, indexed as
    unitigs() numbers them; components are numbered by their smallest unitig), ``stats`` uint64[n components, 4] (root,
    unitigs, keys, abundance), ``verdict`` uint8[n unitigs] (CLEAN_KEEP / CLEAN_COMPONENT), ``table`` (the keys of the kept
    unitigs with their counts, in view order), ``summary``."""
    comp_of: np.ndarray
    stats: np.ndarray
    verdict: np.ndarray
    table: "Table"
    summary: ComponentSummary

    def members(self, c: int) -> np.ndarray:
        """The unitigs of component ``c``, ascending."""
        return np.flatnonzero(self.comp_of == c)

    def to_text(self) -> str:
        """What ``k-mer-count --components`` prints: ``COMPONENT\tROOT\tUNITIGS\tKEYS\tABUND`` lines."""
        return "".join("%d\t%d\t%d\t%d\t%d\n" % ((i,) + tuple(r)) for i, r in enumerate(self.stats.tolist()))


_BUBBLE_FIELDS = ("unitigs", "records", "candidates", "substitutions", "indels", "complex", "reversed", "called_keys")
_RC = bytes.maketrans(b"ACGT", b"TGCA")


@dataclass
class BubbleSummary:
    """The eight words of kmc_unitig_bubbles: unitigs, records (= called arms), bubble candidates, records that are a
    substitution / an indel / complex, records whose major arm is spelled the other way round, the keys of the called arms."""
    unitigs: int
    records: int
    candidates: int
    substitutions: int
    indels: int
    complex: int
    reversed: int
    called_keys: int

    @classmethod
    def from_words(cls, words) -> "BubbleSummary":
        return cls(*[int(w) for w in words])

    def words(self) -> list:
        return [getattr(self, f) for f in _BUBBLE_FIELDS]

    def to_text(self) -> str:
        """``NAME\tVALUE`` lines."""
        return "\n".join("%s\t%d" % (f, getattr(self, f)) for f in _BUBBLE_FIELDS) + "\n"


@dataclass
class Bubbles:
    """What KmerCounter.bubbles returns: ``records`` uint32[n, 8] -- per called arm, ascending: u, its major arm w, the ends p
    and q the pair sits between, lcp, lcs, kind (BUBBLE_SUBST / BUBBLE_INDEL / BUBBLE_COMPLEX, bits 0-1) with BUBBLE_REVERSED
    (bit 2), mism -- ``summary``, and the ``unitigs`` of the same range the ids and positions refer to."""
    records: np.ndarray
    summary: BubbleSummary
    unitigs: "Unitigs"
    k: int

    def __len__(self) -> int:
        return len(self.records)

    def arms(self) -> list:
        """(U, W) per record: the called arm as spelled and its major arm oriented like it."""
        s = self.unitigs.strings()
        out = []
        for r in self.records.tolist():
            w = s[r[1]]
            if r[6] & BUBBLE_REVERSED:
                w = w.encode("ascii").translate(_RC)[::-1].decode("ascii")
            out.append((s[r[0]], w))
        return out

    def alleles(self) -> list:
        """(alt, major) per record: what is left of the two oriented arms between their common prefix and suffix."""
        return [(u[r[4]:len(u) - r[5]], w[r[4]:len(w) - r[5]]) for r, (u, w) in zip(self.records.tolist(), self.arms())]

    def to_text(self) -> str:
        """What ``k-mer-count --variants`` prints: ``INDEX\tKIND\tU\tW\tPOS\tALT\tMAJOR\tA_U/M_U\tA_W/M_W`` lines, KIND one of
        S, I, C, POS the common prefix, ``-`` for an empty allele, then abundance / keys of the two arms."""
        o, a = self.unitigs.offsets, self.unitigs.abund
        m = lambda u: int(o[u + 1]) - int(o[u]) - (self.k - 1)
        return "".join("%d\t%s\t%d\t%d\t%d\t%s\t%s\t%d/%d\t%d/%d\n" % (i, "SIC"[r[6] & 3], r[0], r[1], r[4], alt or "-", maj or "-",
                                                                     int(a[r[0]]), m(r[0]), int(a[r[1]]), m(r[1]))
                       for i, (r, (alt, maj)) in enumerate(zip(self.records.tolist(), self.alleles())))


def parse_fasta(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """Host FASTA reader of libkmc (the reader the reference uses, main.rs:45-46,59-62).
    Returns (bases uint8[n_bases], offsets uint64[n_reads+1])."""
    L = lib()
    rd = _Reads()
    eb = C.create_string_buffer(256)
    rc = L.kmc_parse_fasta(os.fsencode(path), C.byref(rd), eb, 256)
    if rc:
        raise KmcError(rc, eb.value.decode() or L.kmc_status_string(rc).decode())
    try:
        nb, nr = int(rd.n_bases), int(rd.n_reads)
        # (np.ctypeslib.as_array on a POINTER is very slow for GB-sized buffers)
        bases = (np.frombuffer((C.c_uint8 * nb).from_address(C.addressof(rd.bases.contents)), dtype=np.uint8).copy()
                 if nb else np.zeros(0, np.uint8))
        offsets = np.frombuffer((C.c_uint64 * (nr + 1)).from_address(C.addressof(rd.offsets.contents)), dtype=np.uint64).copy()
    finally:
        L.kmc_free_reads(C.byref(rd))
    return bases, offsets


def stream_fasta(path: str, chunk_bytes: int = 0):
    """Streaming form of the host reader: yields (bases, offsets) per chunk of about chunk_bytes of
    FASTA text, each ending at a record boundary (copies: the stream reuses its buffers)."""
    L = lib()
    h = C.c_void_p()
    eb = C.create_string_buffer(256)
    rc = L.kmc_fasta_stream_open(os.fsencode(path), int(chunk_bytes), C.byref(h), eb, 256)
    if rc:
        raise KmcError(rc, eb.value.decode() or L.kmc_status_string(rc).decode())
    try:
        while True:
            rd = _Reads()
            eof = C.c_int(0)
            rc = L.kmc_fasta_stream_next(h, C.byref(rd), C.byref(eof), eb, 256)
            if rc:
                raise KmcError(rc, eb.value.decode() or L.kmc_status_string(rc).decode())
            nb, nr = int(rd.n_bases), int(rd.n_reads)
            bases = (np.frombuffer((C.c_uint8 * nb).from_address(C.addressof(rd.bases.contents)), dtype=np.uint8).copy()
                     if nb else np.zeros(0, np.uint8))
            offsets = np.frombuffer((C.c_uint64 * (nr + 1)).from_address(C.addressof(rd.offsets.contents)), dtype=np.uint64).copy()
            yield bases, offsets
            if eof.value:
                break
    finally:
        L.kmc_fasta_stream_close(h)


# ---------------------------------------------------------------------------------------------
# the counter
# ---------------------------------------------------------------------------------------------
class KmerCounter:
    """One counting context on one GPU (``kmc_ctx``).

    mode=MODE_LR reproduces the reference's computation (27+gap+27, chunk sizes 80..=140,
    main.rs:48-49,63); mode=MODE_CONTIG counts contiguous k-mers.
    """

    def __init__(self, k: int = 31, canonical: bool = True, mode: int = MODE_CONTIG, device: int = 0,
                 algo: int = ALGO_AUTO, capacity_hint: int = 0, stream: Optional[int] = None):
        L = lib()
        self._L = L
        cfg = _Config(C.sizeof(_Config), int(k), int(mode), 1 if canonical else 0, int(device), int(algo),
                      int(capacity_hint), C.c_void_p(stream) if stream else None)
        h = C.c_void_p()
        rc = L.kmc_create(C.byref(h), C.byref(cfg))
        if rc:
            raise KmcError(rc, L.kmc_last_error(None).decode())
        self._h = h
        self.stream = int(stream) if stream else 0  # hipStream_t the ctx runs on (0: its own stream)
        self.k = 54 if mode == MODE_LR else int(k)
        self.mode = mode
        self.canonical = bool(canonical)
        self.device = int(device)

    # -- lifetime --
    def close(self):
        if getattr(self, "_h", None):
            self._L.kmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc: int):
        if rc:
            raise KmcError(rc, self._L.kmc_last_error(self._h).decode())

    # -- feeding --
    def reset(self):
        self._chk(self._L.kmc_reset(self._h))

    def add_batch(self, bases: np.ndarray, offsets: np.ndarray):
        """Host buffers: ASCII bases of all reads concatenated + offsets[n_reads+1]."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = int(offsets.shape[0]) - 1
        self._chk(self._L.kmc_add_batch(self._h, bases.ctypes.data, offsets.ctypes.data, max(n_reads, 0)))

    def add_batch_device(self, d_bases: int, d_offsets: int, n_reads: int, n_bases: int, max_read_len: int = 0):
        """Device-resident buffers given as raw addresses (e.g. torch ``tensor.data_ptr()``)."""
        self._chk(self._L.kmc_add_batch_device(self._h, d_bases, d_offsets, int(n_reads), int(n_bases), int(max_read_len)))

    def add_batch_tensors(self, bases, offsets, max_read_len: int = 0):
        """torch tensors on this ctx's GPU: bases uint8[n_bases], offsets int64[n_reads+1]."""
        assert bases.is_cuda and offsets.is_cuda and bases.is_contiguous() and offsets.is_contiguous()
        self.add_batch_device(bases.data_ptr(), offsets.data_ptr(), offsets.numel() - 1, bases.numel(), max_read_len)

    def merge_pairs_device(self, d_key_hi: int, d_key_lo: int, d_count: int, n: int):
        self._chk(self._L.kmc_merge_pairs_device(self._h, d_key_hi or None, d_key_lo, d_count, int(n)))

    def count_file(self, path: str) -> Tuple[int, int]:
        nd, nt = C.c_uint64(), C.c_uint64()
        self._chk(self._L.kmc_count_file(self._h, os.fsencode(path), C.byref(nd), C.byref(nt)))
        return nd.value, nt.value

    # -- results --
    def finalize(self) -> Tuple[int, int]:
        nd, nt = C.c_uint64(), C.c_uint64()
        self._chk(self._L.kmc_finalize(self._h, C.byref(nd), C.byref(nt)))
        return nd.value, nt.value

    def finalize_async(self):
        """Queue the finalize of a small table and return without waiting (kmc_finalize_async)."""
        self._chk(self._L.kmc_finalize_async(self._h))

    def export(self) -> Table:
        nd, _ = self.finalize()
        hi = np.zeros(nd, np.uint64)
        lo = np.zeros(nd, np.uint64)
        cnt = np.zeros(nd, np.uint64)
        self._chk(self._L.kmc_export(self._h, hi.ctypes.data, lo.ctypes.data, cnt.ctypes.data, nd))
        return Table(hi, lo, cnt, self.k)

    def _device_triple(self, call) -> Tuple[int, int, int]:
        """(d_key_hi or 0, d_key_lo, d_count) of call(key_hi, key_lo, count), which takes the three pointer out-arguments."""
        d = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(call(*map(C.byref, d)))
        return tuple(p.value or 0 for p in d)

    def _sized_table(self, call) -> Table:
        """A host table from an export call of the shape call(key_hi, key_lo, count, cap, n_out): asked for the size
        first (no buffers, cap 0: ERR_ARG with the size in n_out unless the result is empty), then for the entries."""
        n = C.c_uint64()
        rc = call(None, None, None, 0, C.byref(n))
        if rc not in (OK, ERR_ARG) or (rc == ERR_ARG and n.value == 0):
            self._chk(rc)
        nk = n.value
        hi, lo, cnt = np.zeros(nk, np.uint64), np.zeros(nk, np.uint64), np.zeros(nk, np.uint64)
        if nk:
            self._chk(call(hi.ctypes.data, lo.ctypes.data, cnt.ctypes.data, nk, C.byref(n)))
        return Table(hi, lo, cnt, self.k)

    def export_device(self) -> Tuple[int, int, int, int]:
        """(d_key_hi or 0, d_key_lo, d_count, n) of the sorted table of the last finalize."""
        n = C.c_uint64()
        return self._device_triple(lambda *d: self._L.kmc_export_device(self._h, *d, C.byref(n))) + (n.value,)

    def partition_device(self, n_parts: int):
        """Owner-partitioned view for the all-to-all: (part_begin[n_parts+1], d_hi, d_lo, d_cnt)."""
        pb = (C.c_uint64 * (n_parts + 1))()
        d = self._device_triple(lambda *d: self._L.kmc_partition_device(self._h, n_parts, pb, *d))
        return (list(pb),) + d

    # -- after counting: abundance histogram, count-range filter (of the sorted view) --
    def histogram(self, n_bins: int = 10001, min_count: int = 1, max_count: int = 0, return_max: bool = False):
        """Abundance histogram of the sorted view (finalize() first): uint64[n_bins], hist[c] = keys with count c for
        c < n_bins-1, hist[n_bins-1] = keys with count >= n_bins-1; only counts in [min_count, max_count] (max_count 0:
        no upper bound).  return_max=True: (hist, largest count in range)."""
        h = np.zeros(int(n_bins), np.uint64)
        mx = C.c_uint64()
        self._chk(self._L.kmc_histogram(self._h, int(min_count), int(max_count), int(n_bins), h.ctypes.data, C.byref(mx)))
        return (h, mx.value) if return_max else h

    def filter_device(self, min_count: int, max_count: int = 0) -> Tuple[int, int, int, int, int]:
        """(d_key_hi or 0, d_key_lo, d_count, n_kept, kept_total): the keys of the sorted view with count in
        [min_count, max_count], in view order, in ctx-owned device arrays (kmc_filter_device)."""
        n, t = C.c_uint64(), C.c_uint64()
        d = self._device_triple(lambda *d: self._L.kmc_filter_device(self._h, int(min_count), int(max_count), *d, C.byref(n), C.byref(t)))
        return d + (n.value, t.value)

    def export_filtered(self, min_count: int, max_count: int = 0) -> Table:
        """The sorted view restricted to counts in [min_count, max_count] (max_count 0: no upper bound), on the host."""
        return self._sized_table(lambda *out: self._L.kmc_export_filtered(self._h, int(min_count), int(max_count), *out))

    # -- two tables: summary and set operations over the sorted views of self (A) and other (B) --
    @staticmethod
    def _setop_codes(op, counts) -> Tuple[int, int]:
        o = SETOP_NAMES[op] if isinstance(op, str) else int(op)
        m = COUNT_NAMES[counts] if isinstance(counts, str) else int(counts)
        return o, m

    def compare(self, other: "KmerCounter", min_a: int = 1, max_a: int = 0, min_b: int = 1, max_b: int = 0) -> Comparison:
        """kmc_compare: how many keys (with counts in [min_a, max_a] / [min_b, max_b]; max 0: no upper bound) each side
        has, how many both have, and the count sums Jaccard, containment, weighted Jaccard and Bray-Curtis derive from."""
        w = (C.c_uint64 * COMPARE_WORDS)()
        self._chk(self._L.kmc_compare(self._h, other._h, int(min_a), int(max_a), int(min_b), int(max_b), w))
        return Comparison.from_words(list(w))

    def setop_device(self, other: "KmerCounter", op, counts=COUNT_LEFT, min_a: int = 1, max_a: int = 0, min_b: int = 1,
                     max_b: int = 0, return_summary: bool = False):
        """(d_key_hi or 0, d_key_lo, d_count, n_out, total_out) of ``self op other`` in device arrays owned by self
        (kmc_setop_device); op / counts are the SETOP_* / COUNT_* codes or their names.  return_summary=True appends
        the Comparison."""
        o, m = self._setop_codes(op, counts)
        n, t = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * COMPARE_WORDS)()
        r = self._device_triple(lambda *d: self._L.kmc_setop_device(self._h, other._h, o, m, int(min_a), int(max_a), int(min_b), int(max_b), *d,
                                                                    C.byref(n), C.byref(t), w if return_summary else None)) + (n.value, t.value)
        return r + (Comparison.from_words(list(w)),) if return_summary else r

    def setop(self, other: "KmerCounter", op, counts=COUNT_LEFT, min_a: int = 1, max_a: int = 0, min_b: int = 1, max_b: int = 0) -> Table:
        """``self op other`` on the host: intersect / union / subtract with the result count given by ``counts``."""
        o, m = self._setop_codes(op, counts)
        args = (self._h, other._h, o, m, int(min_a), int(max_a), int(min_b), int(max_b))
        return self._sized_table(lambda *out: self._L.kmc_export_setop(*args, *out))

    # -- the table as a de Bruijn graph: neighbour masks, unitig ends, summary (of the sorted view; finalize() first) --
    def graph(self, min_count: int = 1, max_count: int = 0, adj: bool = True):
        """(adj, GraphSummary) of kmc_graph: adj is uint16[n keys of the view] in the order of export() -- bits 0..3 the
        solid right extensions (ACGT), 4..7 the left ones, GRAPH_END_R / GRAPH_END_L "this side ends a unitig", GRAPH_SOLID
        "min_count <= count <= max_count" (max_count 0: no upper bound; other keys get 0) -- or None with adj=False."""
        n = C.c_uint64()
        w = (C.c_uint64 * GRAPH_WORDS)()
        if not adj:
            self._chk(self._L.kmc_graph(self._h, int(min_count), int(max_count), None, 0, C.byref(n), w))
            return None, GraphSummary.from_words(list(w))
        nd = self.export_device()[3]
        out = np.zeros(nd, np.uint16)
        self._chk(self._L.kmc_graph(self._h, int(min_count), int(max_count), out.ctypes.data if nd else None, nd, C.byref(n), w))
        return out, GraphSummary.from_words(list(w))

    def graph_device(self, min_count: int = 1, max_count: int = 0):
        """(d_adj, n, GraphSummary): adj in a ctx-owned device array of n uint16 (kmc_graph_device)."""
        p, n = C.c_void_p(), C.c_uint64()
        w = (C.c_uint64 * GRAPH_WORDS)()
        self._chk(self._L.kmc_graph_device(self._h, int(min_count), int(max_count), C.byref(p), C.byref(n), w))
        return p.value or 0, n.value, GraphSummary.from_words(list(w))

    # -- the unitigs of that graph: sequences, abundances, circular flags (of the sorted view; finalize() first) --
    def unitigs(self, min_count: int = 1, max_count: int = 0) -> "Unitigs":
        """kmc_unitigs: the maximal non-branching paths of the graph of the keys with min_count <= count <= max_count
        (max_count 0: no upper bound), spelled out, in the order of their first keys.  Two calls of the library, one
        computation: the second, which copies, finds the result of the first, which sizes, still in the ctx."""
        nu, nb = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * UNITIG_WORDS)()
        lo, hi = int(min_count), int(max_count)
        self._chk(self._L.kmc_unitigs(self._h, lo, hi, None, 0, None, None, None, 0, C.byref(nu), C.byref(nb), w))
        bases, flags = np.zeros(nb.value, np.uint8), np.zeros(nu.value, np.uint8)
        offsets, abund = np.zeros(nu.value + 1, np.uint64), np.zeros(nu.value, np.uint64)
        self._chk(self._L.kmc_unitigs(self._h, lo, hi, bases.ctypes.data if nb.value else None, nb.value, offsets.ctypes.data,
                                      abund.ctypes.data if nu.value else None, flags.ctypes.data if nu.value else None, nu.value,
                                      C.byref(nu), C.byref(nb), w))
        return Unitigs(bases, offsets, abund, flags, UnitigSummary.from_words(list(w)))

    def unitigs_device(self, min_count: int = 1, max_count: int = 0):
        """(d_bases, d_offsets, d_abund, d_flags, n_unitigs, n_bases, UnitigSummary) of kmc_unitigs_device: ctx-owned device
        arrays; d_bases / d_offsets can be handed to another counter's add_batch_device / profile_device."""
        p = [C.c_void_p() for _ in range(4)]
        nu, nb = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * UNITIG_WORDS)()
        self._chk(self._L.kmc_unitigs_device(self._h, int(min_count), int(max_count), *[C.byref(x) for x in p], C.byref(nu), C.byref(nb), w))
        return tuple(x.value or 0 for x in p) + (nu.value, nb.value, UnitigSummary.from_words(list(w)))

    # -- the links between those unitigs: the edges of the compacted graph (of the sorted view; finalize() first) --
    def unitig_links(self, min_count: int = 1, max_count: int = 0) -> "UnitigLinks":
        """kmc_unitig_links: per unitig end the ends it reaches, for the unitigs of unitigs() with the same range (called
        right after it, the unitigs are not computed again).  Two calls of the library, one computation, as in unitigs()."""
        nu, nl = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * LINK_WORDS)()
        lo, hi = int(min_count), int(max_count)
        self._chk(self._L.kmc_unitig_links(self._h, lo, hi, None, 0, None, 0, C.byref(nu), C.byref(nl), w))
        offsets, to = np.zeros(2 * nu.value + 1, np.uint64), np.zeros(nl.value, np.uint32)
        self._chk(self._L.kmc_unitig_links(self._h, lo, hi, offsets.ctypes.data, 2 * nu.value, to.ctypes.data if nl.value else None,
                                           nl.value, C.byref(nu), C.byref(nl), w))
        return UnitigLinks(offsets, to, LinkSummary.from_words(list(w)))

    def unitig_links_device(self, min_count: int = 1, max_count: int = 0):
        """(d_link_offsets, d_link_to, n_unitigs, n_links, LinkSummary) of kmc_unitig_links_device: ctx-owned device arrays
        of 2 * n_unitigs + 1 uint64 and n_links uint32."""
        p = [C.c_void_p() for _ in range(2)]
        nu, nl = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * LINK_WORDS)()
        self._chk(self._L.kmc_unitig_links_device(self._h, int(min_count), int(max_count), *[C.byref(x) for x in p], C.byref(nu), C.byref(nl), w))
        return tuple(x.value or 0 for x in p) + (nu.value, nl.value, LinkSummary.from_words(list(w)))

    # -- reads threaded through those unitigs: placements, segments, support (of the sorted view; finalize() first) --
    def map_reads_device(self, d_bases: int, d_offsets: int, n_reads: int, n_bases: int, min_count: int = 1, max_count: int = 0):
        """(d_place, d_read_stats, d_seg_offsets, d_segs, d_support, n_segs, n_unitigs, MapSummary) of kmc_unitig_map_device for
        a batch in device memory (raw addresses, laid out as for profile_device): ctx-owned device arrays of n_bases uint64,
        n_reads * 4 uint32, n_reads + 1 uint64, n_segs * 4 uint32 and n_unitigs uint64."""
        p = [C.c_void_p() for _ in range(5)]
        ns, nu = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * MAP_WORDS)()
        self._chk(self._L.kmc_unitig_map_device(self._h, int(min_count), int(max_count), d_bases or None, d_offsets or None, int(n_reads),
                                                int(n_bases), *[C.byref(x) for x in p], C.byref(ns), C.byref(nu), w))
        return tuple(x.value or 0 for x in p) + (ns.value, nu.value, MapSummary.from_words(list(w)))

    def map_reads_tensors(self, bases, offsets, min_count: int = 1, max_count: int = 0):
        """map_reads_device for torch tensors on this ctx's GPU (bases uint8[n_bases], padded as for add_batch_tensors;
        offsets int64[n_reads + 1])."""
        assert bases.is_cuda and offsets.is_cuda and bases.is_contiguous() and offsets.is_contiguous()
        return self.map_reads_device(bases.data_ptr(), offsets.data_ptr(), max(offsets.numel() - 1, 0), bases.numel(), min_count, max_count)

    def map_reads(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 1, max_count: int = 0) -> "ReadMap":
        """kmc_unitig_map_device for a host batch (the batch is not counted): where every window of every read lies in the
        unitigs of unitigs() with the same range.  The batch goes to the device as tensors and the result arrays are read
        back from the ctx, so the library computes once (the host form kmc_unitig_map would need a sizing call first)."""
        import torch
        from .distributed import device_view
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads, n_bases = max(int(offsets.shape[0]) - 1, 0), int(bases.shape[0])
        if n_reads and (int(offsets[0]) != 0 or int(offsets[-1]) != n_bases or (np.diff(offsets.astype(np.int64)) < 0).any()):
            raise ValueError("offsets must start at 0, not decrease, and end at len(bases)")
        if n_reads and int(np.diff(offsets.astype(np.int64)).max()) >= 1 << 32:
            raise KmcError(ERR_ARG, "a read of 2^32 bases or more")
        dev = torch.device("cuda", self.device)
        d_bases = torch.zeros(n_bases + 64, dtype=torch.uint8, device=dev)   # (readable past the end, 16-byte aligned)
        d_bases[:n_bases] = torch.from_numpy(bases.copy())
        d_offs = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        torch.cuda.synchronize(dev)
        dp, ds, do, dg, du, ns, nu, summary = self.map_reads_device(d_bases.data_ptr(), d_offs.data_ptr(), n_reads, n_bases, min_count, max_count)

        def words(ptr, n_bytes):
            return device_view(ptr, (n_bytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:n_bytes].copy()
        return ReadMap(words(dp, 8 * n_bases).view(np.uint64), words(ds, 16 * n_reads).view(np.uint32).reshape(n_reads, MAP_READ_WORDS),
                       words(do, 8 * (n_reads + 1)).view(np.uint64), words(dg, 16 * ns).view(np.uint32).reshape(ns, 4),
                       words(du, 8 * nu).view(np.uint64), summary)

    # -- read walks counted per link record and per unitig (of the sorted view; finalize() first) --
    def transits_device(self, d_bases: int, d_offsets: int, n_reads: int, n_bases: int, min_count: int = 1, max_count: int = 0,
                        min_reads: int = 1, accumulate: bool = False):
        """(d_link_support, d_transit_offsets, d_transit_count, d_verdict, n_unitigs, n_links, n_slots, TransitSummary) of
        kmc_unitig_transits_device for a batch in device memory (raw addresses, laid out as for map_reads_device): ctx-owned
        device arrays of n_links uint64, n_unitigs + 1 uint64, n_slots uint64 and n_unitigs uint8.  ``accumulate`` adds onto
        the result the ctx holds from the last transits call of this view and range."""
        p = [C.c_void_p() for _ in range(4)]
        nu, nl, nsl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * TRANSIT_WORDS)()
        self._chk(self._L.kmc_unitig_transits_device(self._h, int(min_count), int(max_count), int(min_reads), TRANSIT_ACCUMULATE if accumulate else 0,
                                                     d_bases or None, d_offsets or None, int(n_reads), int(n_bases), *[C.byref(x) for x in p],
                                                     C.byref(nu), C.byref(nl), C.byref(nsl), w))
        return tuple(x.value or 0 for x in p) + (nu.value, nl.value, nsl.value, TransitSummary.from_words(list(w)))

    def transits_tensors(self, bases, offsets, min_count: int = 1, max_count: int = 0, min_reads: int = 1, accumulate: bool = False):
        """transits_device for torch tensors on this ctx's GPU (bases uint8[n_bases], padded as for add_batch_tensors;
        offsets int64[n_reads + 1])."""
        assert bases.is_cuda and offsets.is_cuda and bases.is_contiguous() and offsets.is_contiguous()
        return self.transits_device(bases.data_ptr(), offsets.data_ptr(), max(offsets.numel() - 1, 0), bases.numel(), min_count, max_count,
                                    min_reads, accumulate)

    def transits(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 1, max_count: int = 0, min_reads: int = 1,
                 accumulate: bool = False) -> "Transits":
        """kmc_unitig_transits_device for a host batch (the batch is not counted): how many of its reads walk every link
        record of unitig_links() with the same range, which way into a unitig goes with which way out, and a verdict per
        repeat.  The batch goes to the device as tensors and the result arrays are read back from the ctx, so the library
        computes once; the links it returns with them are the ones it counted on."""
        import torch
        from .distributed import device_view
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads, n_bases = max(int(offsets.shape[0]) - 1, 0), int(bases.shape[0])
        if n_reads and (int(offsets[0]) != 0 or int(offsets[-1]) != n_bases or (np.diff(offsets.astype(np.int64)) < 0).any()):
            raise ValueError("offsets must start at 0, not decrease, and end at len(bases)")
        if n_reads and int(np.diff(offsets.astype(np.int64)).max()) >= 1 << 32:
            raise KmcError(ERR_ARG, "a read of 2^32 bases or more")
        dev = torch.device("cuda", self.device)
        d_bases = torch.zeros(n_bases + 64, dtype=torch.uint8, device=dev)   # (readable past the end, 16-byte aligned)
        d_bases[:n_bases] = torch.from_numpy(bases.copy())
        d_offs = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        torch.cuda.synchronize(dev)
        ds, do, dc, dv, nu, nl, nsl, summary = self.transits_device(d_bases.data_ptr(), d_offs.data_ptr(), n_reads, n_bases, min_count, max_count,
                                                                    min_reads, accumulate)

        def words(ptr, n_bytes):
            return device_view(ptr, (n_bytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:n_bytes].copy()
        got = (words(ds, 8 * nl).view(np.uint64), words(do, 8 * (nu + 1)).view(np.uint64), words(dc, 8 * nsl).view(np.uint64), words(dv, nu))
        return Transits(*got, summary, self.unitig_links(min_count, max_count))   # (the held links: copied, not computed)

    # -- pair evidence: the unitig ends the mates of a pair connect, insert sizes (of the sorted view; finalize() first) --
    def pair_links_device(self, d_bases: int, d_offsets: int, n_reads: int, n_bases: int, min_count: int = 1, max_count: int = 0,
                          n_bins: int = 1024, accumulate: bool = False):
        """(d_pair_class, d_pair_ends, d_pair_value, d_rec_ends, d_rec_count, d_rec_sum, d_rec_min, d_rec_max, d_insert_hist,
        n_pairs, n_records, PairSummary) of kmc_unitig_pairs_device for a batch in device memory (raw addresses, laid out as
        for map_reads_device, reads 2i and 2i + 1 the mates of pair i): ctx-owned device arrays.  ``accumulate`` adds onto the
        result the ctx holds from the last pairs call of this view, range and n_bins."""
        p = [C.c_void_p() for _ in range(9)]
        npairs, nrec = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * PAIR_WORDS)()
        self._chk(self._L.kmc_unitig_pairs_device(self._h, int(min_count), int(max_count), int(n_bins), PAIR_ACCUMULATE if accumulate else 0,
                                                  d_bases or None, d_offsets or None, int(n_reads), int(n_bases), *[C.byref(x) for x in p],
                                                  C.byref(npairs), C.byref(nrec), w))
        return tuple(x.value or 0 for x in p) + (npairs.value, nrec.value, PairSummary.from_words(list(w)))

    def pair_links_tensors(self, bases, offsets, min_count: int = 1, max_count: int = 0, n_bins: int = 1024, accumulate: bool = False):
        """pair_links_device for torch tensors on this ctx's GPU (bases uint8[n_bases], padded as for add_batch_tensors;
        offsets int64[n_reads + 1])."""
        assert bases.is_cuda and offsets.is_cuda and bases.is_contiguous() and offsets.is_contiguous()
        return self.pair_links_device(bases.data_ptr(), offsets.data_ptr(), max(offsets.numel() - 1, 0), bases.numel(), min_count, max_count,
                                      n_bins, accumulate)

    def pair_links(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 1, max_count: int = 0, n_bins: int = 1024,
                   accumulate: bool = False) -> "PairLinks":
        """kmc_unitig_pairs_device for a host batch of interleaved mates (the batch is not counted): the class of every pair
        on the unitigs of unitigs() with the same range, the records of the pairs that span two unitigs, and the insert
        histogram of those that lie on one.  The batch goes to the device as tensors and the result arrays are read back from
        the ctx, so the library computes once."""
        import torch
        from .distributed import device_view
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads, n_bases = max(int(offsets.shape[0]) - 1, 0), int(bases.shape[0])
        if n_reads and (int(offsets[0]) != 0 or int(offsets[-1]) != n_bases or (np.diff(offsets.astype(np.int64)) < 0).any()):
            raise ValueError("offsets must start at 0, not decrease, and end at len(bases)")
        if n_reads and int(np.diff(offsets.astype(np.int64)).max()) >= 1 << 32:
            raise KmcError(ERR_ARG, "a read of 2^32 bases or more")
        dev = torch.device("cuda", self.device)
        d_bases = torch.zeros(n_bases + 64, dtype=torch.uint8, device=dev)   # (readable past the end, 16-byte aligned)
        d_bases[:n_bases] = torch.from_numpy(bases.copy())
        d_offs = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        torch.cuda.synchronize(dev)
        *ptr, n_pairs, n_rec, summary = self.pair_links_device(d_bases.data_ptr(), d_offs.data_ptr(), n_reads, n_bases, min_count, max_count,
                                                               n_bins, accumulate)

        def words(p, n_bytes):
            return device_view(p, (n_bytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:n_bytes].copy()
        u64s = lambda p, n: words(p, 8 * n).view(np.uint64)
        return PairLinks(words(ptr[0], n_pairs), words(ptr[1], 8 * n_pairs).view(np.uint32).reshape(n_pairs, 2), u64s(ptr[2], n_pairs),
                         words(ptr[3], 8 * n_rec).view(np.uint32).reshape(n_rec, 2), u64s(ptr[4], n_rec), u64s(ptr[5], n_rec), u64s(ptr[6], n_rec),
                         u64s(ptr[7], n_rec), u64s(ptr[8], int(n_bins)), summary)

    # -- the counted walks acted on: contigs (after unitigs / unitig_links / transits of the same range) --
    def contigs(self, min_count: int = 1, max_count: int = 0, min_reads: int = 1, min_support: int = 0) -> "Contigs":
        """kmc_unitig_contigs: the chains of unitigs that remain once every repeat the held transit counts resolve (under
        ``min_reads``) has one copy per matched way through it and, with ``min_support``, every link record below that support
        is ignored at the ends of single-copy unitigs.  The ctx must hold the unitigs, links and transits of this range
        (transits() leaves all three).  Two calls of the library, one computation, as in unitigs()."""
        n = [C.c_uint64() for _ in range(3)]
        w = (C.c_uint64 * CONTIG_WORDS)()
        a = (int(min_count), int(max_count), int(min_reads), int(min_support))
        self._chk(self._L.kmc_unitig_contigs(self._h, *a, None, 0, None, None, None, None, 0, None, 0, *[C.byref(x) for x in n], w))
        nc, nn, nb = (x.value for x in n)
        bases, flags, path = np.zeros(nb, np.uint8), np.zeros(nc, np.uint8), np.zeros(nn, np.uint32)
        offsets, path_offsets, abund = np.zeros(nc + 1, np.uint64), np.zeros(nc + 1, np.uint64), np.zeros(nc, np.uint64)
        self._chk(self._L.kmc_unitig_contigs(self._h, *a, bases.ctypes.data if nb else None, nb, offsets.ctypes.data, path_offsets.ctypes.data,
                                             abund.ctypes.data if nc else None, flags.ctypes.data if nc else None, nc,
                                             path.ctypes.data if nn else None, nn, *[C.byref(x) for x in n], w))
        return Contigs(bases, offsets, path_offsets, path, abund, flags, ContigSummary.from_words(list(w)))

    def contigs_device(self, min_count: int = 1, max_count: int = 0, min_reads: int = 1, min_support: int = 0):
        """(d_bases, d_offsets, d_path_offsets, d_path, d_abund, d_flags, n_contigs, n_nodes, n_bases, ContigSummary) of
        kmc_unitig_contigs_device: ctx-owned device arrays; d_bases / d_offsets can be handed to another counter's
        add_batch_device."""
        p = [C.c_void_p() for _ in range(6)]
        n = [C.c_uint64() for _ in range(3)]
        w = (C.c_uint64 * CONTIG_WORDS)()
        self._chk(self._L.kmc_unitig_contigs_device(self._h, int(min_count), int(max_count), int(min_reads), int(min_support),
                                                    *[C.byref(x) for x in p], *[C.byref(x) for x in n], w))
        return tuple(x.value or 0 for x in p) + tuple(x.value for x in n) + (ContigSummary.from_words(list(w)),)

    # -- reads corrected against the solid keys of the table (of the sorted view; finalize() first) --
    def correct_reads_device(self, d_bases: int, d_offsets: int, n_reads: int, n_bases: int, min_count: int = 2, max_count: int = 0):
        """(d_corrected, d_read_stats, d_cand_offsets, d_cands, n_cands, CorrectSummary) of kmc_correct_device for a batch in
        device memory (raw addresses, laid out as for profile_device): ctx-owned device arrays of n_bases uint8 (padded as
        add_batch_device asks), n_reads * 4 uint32, n_reads + 1 uint64 and n_cands * 4 uint32."""
        p = [C.c_void_p() for _ in range(4)]
        nc = C.c_uint64()
        w = (C.c_uint64 * CORRECT_WORDS)()
        self._chk(self._L.kmc_correct_device(self._h, int(min_count), int(max_count), d_bases or None, d_offsets or None, int(n_reads), int(n_bases),
                                             *[C.byref(x) for x in p], C.byref(nc), w))
        return tuple(x.value or 0 for x in p) + (nc.value, CorrectSummary.from_words(list(w)))

    def correct_reads_tensors(self, bases, offsets, min_count: int = 2, max_count: int = 0):
        """correct_reads_device for torch tensors on this ctx's GPU (bases uint8[n_bases], padded as for add_batch_tensors;
        offsets int64[n_reads + 1])."""
        assert bases.is_cuda and offsets.is_cuda and bases.is_contiguous() and offsets.is_contiguous()
        return self.correct_reads_device(bases.data_ptr(), offsets.data_ptr(), max(offsets.numel() - 1, 0), bases.numel(), min_count, max_count)

    def correct_reads(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 2, max_count: int = 0) -> "CorrectedReads":
        """kmc_correct_device for a host batch (the batch is not counted): every substitution error that leaves one clean run
        of weak windows is replaced by the one base that makes all windows over it solid (count in min_count..max_count).
        The batch goes to the device as tensors and the result arrays are read back from the ctx."""
        import torch
        from .distributed import device_view
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads, n_bases = max(int(offsets.shape[0]) - 1, 0), int(bases.shape[0])
        if n_reads and (int(offsets[0]) != 0 or int(offsets[-1]) != n_bases or (np.diff(offsets.astype(np.int64)) < 0).any()):
            raise ValueError("offsets must start at 0, not decrease, and end at len(bases)")
        if n_reads and int(np.diff(offsets.astype(np.int64)).max()) >= 1 << 32:
            raise KmcError(ERR_ARG, "a read of 2^32 bases or more")
        dev = torch.device("cuda", self.device)
        d_bases = torch.zeros(n_bases + 64, dtype=torch.uint8, device=dev)   # (readable past the end, 16-byte aligned)
        d_bases[:n_bases] = torch.from_numpy(bases.copy())
        d_offs = torch.from_numpy(offsets.view(np.int64).copy()).to(dev)
        torch.cuda.synchronize(dev)
        db, ds, do, dc, nc, summary = self.correct_reads_device(d_bases.data_ptr(), d_offs.data_ptr(), n_reads, n_bases, min_count, max_count)

        def words(ptr, n_bytes):
            return device_view(ptr, (n_bytes + 7) // 8, dev).cpu().numpy().view(np.uint8)[:n_bytes].copy()
        out = words(db, n_bases) if n_reads else bases.copy()
        return CorrectedReads(out, offsets.copy() if n_reads else np.zeros(1, np.uint64), words(ds, 16 * n_reads).view(np.uint32).reshape(n_reads, CORRECT_READ_WORDS),
                              words(do, 8 * (n_reads + 1)).view(np.uint64), words(dc, 16 * nc).view(np.uint32).reshape(nc, 4), summary)

    # -- reads trimmed and filtered by their strong windows (of the sorted view; finalize() first) --
    def trim_reads_device(self, d_bases: int, d_offsets: int, n_reads: int, n_bases: int, min_count: int = 1, max_count: int = 0,
                          mode: int = TRIM_LONGEST, flags: int = 0, min_strong: int = 0, min_permille: int = 0, min_len: int = 0):
        """(d_out_bases, d_out_offsets, d_origin, d_read_stats, d_verdict, n_out, n_out_bases, TrimSummary) of kmc_trim_device
        for a batch in device memory (raw addresses, laid out as for profile_device): ctx-owned device arrays of n_out_bases
        uint8 (padded as add_batch_device asks), n_out + 1 uint64, n_out uint64, n_reads * 4 uint32 and n_reads uint8."""
        p = [C.c_void_p() for _ in range(5)]
        no, nb = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * TRIM_WORDS)()
        self._chk(self._L.kmc_trim_device(self._h, int(min_count), int(max_count), int(mode), int(flags), int(min_strong), int(min_permille),
                                          int(min_len), d_bases or None, d_offsets or None, int(n_reads), int(n_bases),
                                          *[C.byref(x) for x in p], C.byref(no), C.byref(nb), w))
        return tuple(x.value or 0 for x in p) + (no.value, nb.value, TrimSummary.from_words(list(w)))

    def trim_reads_tensors(self, bases, offsets, min_count: int = 1, max_count: int = 0, mode: int = TRIM_LONGEST, flags: int = 0,
                           min_strong: int = 0, min_permille: int = 0, min_len: int = 0):
        """trim_reads_device for torch tensors on this ctx's GPU (bases uint8[n_bases], padded as for add_batch_tensors;
        offsets int64[n_reads + 1])."""
        assert bases.is_cuda and offsets.is_cuda and bases.is_contiguous() and offsets.is_contiguous()
        return self.trim_reads_device(bases.data_ptr(), offsets.data_ptr(), max(offsets.numel() - 1, 0), bases.numel(), min_count, max_count,
                                      mode, flags, min_strong, min_permille, min_len)

    def trim_reads(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 1, max_count: int = 0, mode: int = TRIM_LONGEST,
                   flags: int = 0, min_strong: int = 0, min_permille: int = 0, min_len: int = 0) -> "TrimmedReads":
        """kmc_trim for a host batch (the batch is not counted): per read the span the table supports (mode: the whole read,
        from the first to the last strong window, or the longest run of strong windows; strong = count in
        min_count..max_count), the reads that pass min_strong / min_permille / min_len (flags: pairs, inverted) and their
        spans as a new batch."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = max(int(offsets.shape[0]) - 1, 0)
        if n_reads and int(offsets[-1]) != int(bases.shape[0]):
            raise ValueError("offsets must end at len(bases)")
        args = (int(min_count), int(max_count), int(mode), int(flags), int(min_strong), int(min_permille), int(min_len),
                bases.ctypes.data if n_reads else None, offsets.ctypes.data if n_reads else None, n_reads)
        no, nb = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * TRIM_WORDS)()
        self._chk(self._L.kmc_trim(self._h, *args, None, 0, None, None, 0, None, None, C.byref(no), C.byref(nb), None))
        out, oo, org = np.zeros(nb.value, np.uint8), np.zeros(no.value + 1, np.uint64), np.zeros(no.value, np.uint64)
        stats, verdict = np.zeros((n_reads, TRIM_READ_WORDS), np.uint32), np.zeros(n_reads, np.uint8)
        self._chk(self._L.kmc_trim(self._h, *args, out.ctypes.data, nb.value, oo.ctypes.data, org.ctypes.data, no.value, stats.ctypes.data,
                                   verdict.ctypes.data, C.byref(no), C.byref(nb), w))
        return TrimmedReads(out, oo, org, stats, verdict, TrimSummary.from_words(list(w)))

    # -- read depth normalised: a percentile depth per read, deep reads sampled down (of the sorted view; finalize() first) --
    def normalize_reads_device(self, d_bases: int, d_offsets: int, n_reads: int, n_bases: int, target: int = 0, permille: int = 500,
                               min_depth: int = 0, seed: int = 0, flags: int = 0):
        """(d_out_bases, d_out_offsets, d_origin, d_read_stats, d_verdict, n_out, n_out_bases, NormalizeSummary) of
        kmc_normalize_device for a batch in device memory (raw addresses, laid out as for profile_device): ctx-owned device
        arrays of n_out_bases uint8 (padded as add_batch_device asks), n_out + 1 uint64, n_out uint64, n_reads * 4 uint32 and
        n_reads uint8."""
        p = [C.c_void_p() for _ in range(5)]
        no, nb = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * NORMALIZE_WORDS)()
        self._chk(self._L.kmc_normalize_device(self._h, int(permille), int(target), int(min_depth), int(seed), int(flags), d_bases or None,
                                               d_offsets or None, int(n_reads), int(n_bases), *[C.byref(x) for x in p], C.byref(no), C.byref(nb), w))
        return tuple(x.value or 0 for x in p) + (no.value, nb.value, NormalizeSummary.from_words(list(w)))

    def normalize_reads_tensors(self, bases, offsets, target: int = 0, permille: int = 500, min_depth: int = 0, seed: int = 0, flags: int = 0):
        """normalize_reads_device for torch tensors on this ctx's GPU (bases uint8[n_bases], padded as for add_batch_tensors;
        offsets int64[n_reads + 1])."""
        assert bases.is_cuda and offsets.is_cuda and bases.is_contiguous() and offsets.is_contiguous()
        return self.normalize_reads_device(bases.data_ptr(), offsets.data_ptr(), max(offsets.numel() - 1, 0), bases.numel(), target, permille,
                                           min_depth, seed, flags)

    def normalize_reads(self, bases: np.ndarray, offsets: np.ndarray, target: int = 0, permille: int = 500, min_depth: int = 0, seed: int = 0,
                        flags: int = 0) -> "NormalizedReads":
        """kmc_normalize for a host batch (the batch is not counted): per read its depth, the permille-th thousandth of the
        sorted counts of its valid windows (500: the lower median); units (reads, or pairs with NORM_PAIRED) below min_depth
        are dropped, units above target are kept with probability target / depth (seed), and the emitted reads (NORM_INVERT:
        the others) come back whole as a new batch."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = max(int(offsets.shape[0]) - 1, 0)
        if n_reads and int(offsets[-1]) != int(bases.shape[0]):
            raise ValueError("offsets must end at len(bases)")
        args = (int(permille), int(target), int(min_depth), int(seed), int(flags), bases.ctypes.data if n_reads else None,
                offsets.ctypes.data if n_reads else None, n_reads)
        no, nb = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * NORMALIZE_WORDS)()
        self._chk(self._L.kmc_normalize(self._h, *args, None, 0, None, None, 0, None, None, C.byref(no), C.byref(nb), None))
        out, oo, org = np.zeros(nb.value, np.uint8), np.zeros(no.value + 1, np.uint64), np.zeros(no.value, np.uint64)
        stats, verdict = np.zeros((n_reads, NORMALIZE_READ_WORDS), np.uint32), np.zeros(n_reads, np.uint8)
        self._chk(self._L.kmc_normalize(self._h, *args, out.ctypes.data, nb.value, oo.ctypes.data, org.ctypes.data, no.value, stats.ctypes.data,
                                        verdict.ctypes.data, C.byref(no), C.byref(nb), w))
        return NormalizedReads(out, oo, org, stats, verdict, NormalizeSummary.from_words(list(w)))

    # -- that graph cleaned: tips clipped, islands dropped (of the sorted view; finalize() first) --
    def _clean_limits(self, max_tip_keys, max_island_keys) -> Tuple[int, int]:
        return (self.k if max_tip_keys is None else int(max_tip_keys)), (self.k if max_island_keys is None else int(max_island_keys))

    def clean_unitigs(self, min_count: int = 1, max_count: int = 0, max_tip_keys: Optional[int] = None,
                      max_island_keys: Optional[int] = None) -> "CleanedUnitigs":
        """kmc_unitig_clean: the verdict per unitig of unitigs() / unitig_links() with the same range -- dead-end arms of at
        most max_tip_keys keys that lose against a sibling are tips, unconnected unitigs of at most max_island_keys keys
        islands (None: k; 0: none) -- and the table of the keys of the kept unitigs.  Two calls, one computation."""
        tip, isl = self._clean_limits(max_tip_keys, max_island_keys)
        nk, nu = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * CLEAN_WORDS)()
        lo, hi = int(min_count), int(max_count)
        self._chk(self._L.kmc_unitig_clean(self._h, lo, hi, tip, isl, None, None, None, 0, None, 0, C.byref(nk), C.byref(nu), w))
        khi, klo, cnt = (np.zeros(nk.value, np.uint64) for _ in range(3))
        verdict = np.zeros(nu.value, np.uint8)
        self._chk(self._L.kmc_unitig_clean(self._h, lo, hi, tip, isl, khi.ctypes.data if nk.value else None, klo.ctypes.data if nk.value else None,
                                           cnt.ctypes.data if nk.value else None, nk.value, verdict.ctypes.data if nu.value else None, nu.value,
                                           C.byref(nk), C.byref(nu), w))
        return CleanedUnitigs(Table(khi, klo, cnt, self.k), verdict, CleanSummary.from_words(list(w)))

    def clean_unitigs_device(self, min_count: int = 1, max_count: int = 0, max_tip_keys: Optional[int] = None,
                             max_island_keys: Optional[int] = None):
        """(d_key_hi or 0, d_key_lo, d_count, d_verdict, n_kept, n_unitigs, CleanSummary) of kmc_unitig_clean_device: ctx-owned
        device arrays; the first three can be handed to another counter's merge_pairs_device."""
        tip, isl = self._clean_limits(max_tip_keys, max_island_keys)
        p = [C.c_void_p() for _ in range(4)]
        nk, nu = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * CLEAN_WORDS)()
        self._chk(self._L.kmc_unitig_clean_device(self._h, int(min_count), int(max_count), tip, isl, *[C.byref(x) for x in p], C.byref(nk), C.byref(nu), w))
        return tuple(x.value or 0 for x in p) + (nk.value, nu.value, CleanSummary.from_words(list(w)))

    def clean_into(self, dst: "KmerCounter", min_count: int = 1, max_count: int = 0, max_tip_keys: Optional[int] = None,
                   max_island_keys: Optional[int] = None) -> "CleanSummary":
        """kmc_unitig_clean_into: the kept keys of self merged into dst's table (dst is not finalized)."""
        tip, isl = self._clean_limits(max_tip_keys, max_island_keys)
        w = (C.c_uint64 * CLEAN_WORDS)()
        self._chk(self._L.kmc_unitig_clean_into(self._h, dst._h, int(min_count), int(max_count), tip, isl, w))
        return CleanSummary.from_words(list(w))

    def cleaned(self, min_count: int = 1, max_count: int = 0, max_tip_keys: Optional[int] = None, max_island_keys: Optional[int] = None,
                rounds: int = 1):
        """(KmerCounter, [CleanSummary per round run]): a new finalized counter on this device, same k and canonical, that
        holds this table cleaned ``rounds`` times -- round 2 and later run on the previous round's counter with the same
        range.  Stops early after a round that removes nothing.  Intermediate counters are closed; self is left as it is."""
        if rounds < 1:
            raise ValueError("rounds must be at least 1")
        src, out = self, []
        for _ in range(int(rounds)):
            dst = KmerCounter(k=self.k, canonical=self.canonical, mode=self.mode, device=self.device)
            try:
                out.append(src.clean_into(dst, min_count, max_count, max_tip_keys, max_island_keys))
                dst.finalize()
            except Exception:
                dst.close()
                if src is not self:
                    src.close()
                raise
            if src is not self:
                src.close()
            src = dst
            if out[-1].removed == 0:
                break
        return src, out

    # -- that graph as a whole: connected components labelled, the small ones dropped --
    def components(self, min_count: int = 1, max_count: int = 0, max_component_keys: int = 0) -> "Components":
        """kmc_unitig_components: the connected component of every unitig of unitigs() / unitig_links() with the same range,
        root / unitigs / keys / abundance per component, and the table without the components of at most
        max_component_keys keys (0: none is dropped).  Two calls, one computation."""
        lo, hi, lim = int(min_count), int(max_count), int(max_component_keys)
        nc, nu, nk = C.c_uint64(), C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * COMPONENT_WORDS)()
        self._chk(self._L.kmc_unitig_components(self._h, lo, hi, lim, None, None, 0, None, 0, None, None, None, 0, C.byref(nc), C.byref(nu),
                                                C.byref(nk), w))
        khi, klo, cnt = (np.zeros(nk.value, np.uint64) for _ in range(3))
        comp_of, verdict = np.zeros(nu.value, np.uint32), np.zeros(nu.value, np.uint8)
        stats = np.zeros((nc.value, COMPONENT_STAT_WORDS), np.uint64)
        ptr = lambda a: a.ctypes.data if a.size else None
        self._chk(self._L.kmc_unitig_components(self._h, lo, hi, lim, ptr(comp_of), ptr(verdict), nu.value, ptr(stats), nc.value, ptr(khi), ptr(klo),
                                                ptr(cnt), nk.value, C.byref(nc), C.byref(nu), C.byref(nk), w))
        return Components(comp_of, stats, verdict, Table(khi, klo, cnt, self.k), ComponentSummary.from_words(list(w)))

    def components_device(self, min_count: int = 1, max_count: int = 0, max_component_keys: int = 0):
        """(d_comp_of, d_comp_stats, d_verdict, d_key_hi or 0, d_key_lo, d_count, n_comps, n_unitigs, n_kept, ComponentSummary)
        of kmc_unitig_components_device: ctx-owned device arrays; the three of the kept table can be handed to another
        counter's merge_pairs_device."""
        p = [C.c_void_p() for _ in range(6)]
        nc, nu, nk = C.c_uint64(), C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * COMPONENT_WORDS)()
        self._chk(self._L.kmc_unitig_components_device(self._h, int(min_count), int(max_count), int(max_component_keys), *[C.byref(x) for x in p],
                                                       C.byref(nc), C.byref(nu), C.byref(nk), w))
        return tuple(x.value or 0 for x in p) + (nc.value, nu.value, nk.value, ComponentSummary.from_words(list(w)))

    def components_into(self, dst: "KmerCounter", min_count: int = 1, max_count: int = 0, max_component_keys: int = 0) -> "ComponentSummary":
        """kmc_unitig_components_into: the keys of self outside small components merged into dst's table (dst is not finalized)."""
        w = (C.c_uint64 * COMPONENT_WORDS)()
        self._chk(self._L.kmc_unitig_components_into(self._h, dst._h, int(min_count), int(max_count), int(max_component_keys), w))
        return ComponentSummary.from_words(list(w))

    # -- its bubbles reported as variants: which arm lost against which, between which ends, and how the two differ --
    def bubbles(self, min_count: int = 1, max_count: int = 0, max_bubble_keys: Optional[int] = None) -> "Bubbles":
        """kmc_unitig_bubbles: one record per unitig that simplify_unitigs with the same range and bubble limit (None: k; 0:
        none) would pop -- the arm it lost against, the two ends between which the pair sits, and the difference of the two
        spellings as common prefix, common suffix, kind and mismatches.  Two calls, one computation; the unitigs of the range
        come along (they are held by the ctx: nothing is computed again for them)."""
        lo, hi = int(min_count), int(max_count)
        lim = self.k if max_bubble_keys is None else int(max_bubble_keys)
        nr, nu = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * BUBBLE_WORDS)()
        self._chk(self._L.kmc_unitig_bubbles(self._h, lo, hi, lim, None, 0, C.byref(nr), C.byref(nu), w))
        unitigs = self.unitigs(lo, hi)
        rec = np.zeros((nr.value, BUBBLE_RECORD_WORDS), np.uint32)
        self._chk(self._L.kmc_unitig_bubbles(self._h, lo, hi, lim, rec.ctypes.data if nr.value else None, nr.value, C.byref(nr), C.byref(nu), w))
        return Bubbles(rec, BubbleSummary.from_words(list(w)), unitigs, self.k)

    def bubbles_device(self, min_count: int = 1, max_count: int = 0, max_bubble_keys: Optional[int] = None):
        """(d_records, n_records, n_unitigs, BubbleSummary) of kmc_unitig_bubbles_device: a ctx-owned device array of
        n_records * 8 uint32."""
        lim = self.k if max_bubble_keys is None else int(max_bubble_keys)
        p = C.c_void_p()
        nr, nu = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * BUBBLE_WORDS)()
        self._chk(self._L.kmc_unitig_bubbles_device(self._h, int(min_count), int(max_count), lim, C.byref(p), C.byref(nr), C.byref(nu), w))
        return p.value or 0, nr.value, nu.value, BubbleSummary.from_words(list(w))

    # -- and simple bubbles popped: the arm of a fork-and-rejoin that loses against its parallel arm --
    def _simplify_limits(self, max_tip_keys, max_island_keys, max_bubble_keys) -> Tuple[int, int, int]:
        return self._clean_limits(max_tip_keys, max_island_keys) + (self.k if max_bubble_keys is None else int(max_bubble_keys),)

    def simplify_unitigs(self, min_count: int = 1, max_count: int = 0, max_tip_keys: Optional[int] = None,
                         max_island_keys: Optional[int] = None, max_bubble_keys: Optional[int] = None) -> "SimplifiedUnitigs":
        """kmc_unitig_simplify: clean_unitigs with a fourth verdict -- a unitig of at most max_bubble_keys keys (None: k; 0:
        none) with one link at each end that loses against a parallel unitig between the same two ends is a bubble.  The
        counts of a popped arm are not added to the survivor.  Two calls, one computation."""
        tip, isl, bub = self._simplify_limits(max_tip_keys, max_island_keys, max_bubble_keys)
        nk, nu = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * SIMPLIFY_WORDS)()
        lo, hi = int(min_count), int(max_count)
        self._chk(self._L.kmc_unitig_simplify(self._h, lo, hi, tip, isl, bub, None, None, None, 0, None, 0, C.byref(nk), C.byref(nu), w))
        khi, klo, cnt = (np.zeros(nk.value, np.uint64) for _ in range(3))
        verdict = np.zeros(nu.value, np.uint8)
        self._chk(self._L.kmc_unitig_simplify(self._h, lo, hi, tip, isl, bub, khi.ctypes.data if nk.value else None,
                                              klo.ctypes.data if nk.value else None, cnt.ctypes.data if nk.value else None, nk.value,
                                              verdict.ctypes.data if nu.value else None, nu.value, C.byref(nk), C.byref(nu), w))
        return SimplifiedUnitigs(Table(khi, klo, cnt, self.k), verdict, SimplifySummary.from_words(list(w)))

    def simplify_unitigs_device(self, min_count: int = 1, max_count: int = 0, max_tip_keys: Optional[int] = None,
                                max_island_keys: Optional[int] = None, max_bubble_keys: Optional[int] = None):
        """(d_key_hi or 0, d_key_lo, d_count, d_verdict, n_kept, n_unitigs, SimplifySummary) of kmc_unitig_simplify_device:
        ctx-owned device arrays, as clean_unitigs_device gives them."""
        tip, isl, bub = self._simplify_limits(max_tip_keys, max_island_keys, max_bubble_keys)
        p = [C.c_void_p() for _ in range(4)]
        nk, nu = C.c_uint64(), C.c_uint64()
        w = (C.c_uint64 * SIMPLIFY_WORDS)()
        self._chk(self._L.kmc_unitig_simplify_device(self._h, int(min_count), int(max_count), tip, isl, bub, *[C.byref(x) for x in p],
                                                     C.byref(nk), C.byref(nu), w))
        return tuple(x.value or 0 for x in p) + (nk.value, nu.value, SimplifySummary.from_words(list(w)))

    def simplify_into(self, dst: "KmerCounter", min_count: int = 1, max_count: int = 0, max_tip_keys: Optional[int] = None,
                      max_island_keys: Optional[int] = None, max_bubble_keys: Optional[int] = None) -> "SimplifySummary":
        """kmc_unitig_simplify_into: the kept keys of self merged into dst's table (dst is not finalized)."""
        tip, isl, bub = self._simplify_limits(max_tip_keys, max_island_keys, max_bubble_keys)
        w = (C.c_uint64 * SIMPLIFY_WORDS)()
        self._chk(self._L.kmc_unitig_simplify_into(self._h, dst._h, int(min_count), int(max_count), tip, isl, bub, w))
        return SimplifySummary.from_words(list(w))

    def simplified(self, min_count: int = 1, max_count: int = 0, max_tip_keys: Optional[int] = None, max_island_keys: Optional[int] = None,
                   max_bubble_keys: Optional[int] = None, rounds: int = 1):
        """(KmerCounter, [SimplifySummary per round run]): cleaned() with bubbles popped in every round.  Stops early after a
        round that removes nothing.  Intermediate counters are closed; self is left as it is."""
        if rounds < 1:
            raise ValueError("rounds must be at least 1")
        src, out = self, []
        for _ in range(int(rounds)):
            dst = KmerCounter(k=self.k, canonical=self.canonical, mode=self.mode, device=self.device)
            try:
                out.append(src.simplify_into(dst, min_count, max_count, max_tip_keys, max_island_keys, max_bubble_keys))
                dst.finalize()
            except Exception:
                dst.close()
                if src is not self:
                    src.close()
                raise
            if src is not self:
                src.close()
            src = dst
            if out[-1].removed == 0:
                break
        return src, out

    # -- asking the table: key lookups and per-read profiles (of the sorted view; finalize() first) --
    def query(self, key_lo, key_hi=None) -> np.ndarray:
        """uint64 counts of the given packed keys (0 = absent), looked up as given; key_hi None: high words zero."""
        lo = np.ascontiguousarray(key_lo, dtype=np.uint64).ravel()
        hi = None if key_hi is None else np.ascontiguousarray(key_hi, dtype=np.uint64).ravel()
        if hi is not None and hi.shape != lo.shape:
            raise ValueError("key_hi and key_lo differ in length")
        out = np.zeros(lo.shape[0], np.uint64)
        self._chk(self._L.kmc_query(self._h, hi.ctypes.data if hi is not None else None, lo.ctypes.data, lo.shape[0], out.ctypes.data))
        return out

    def query_kmers(self, kmers: Iterable) -> np.ndarray:
        """Counts of ASCII k-mers (str or bytes, each of this ctx's key length), encoded with the ctx's canonical setting."""
        keys = [encode_key(km, self.canonical) for km in kmers]
        hi = np.array([h for h, _ in keys], np.uint64)
        lo = np.array([l for _, l in keys], np.uint64)
        return self.query(lo, hi)

    def query_device(self, d_key_hi: int, d_key_lo: int, n_keys: int, d_count: int):
        """Device arrays given as raw addresses (d_key_hi 0: high words zero); asynchronous on the ctx stream."""
        self._chk(self._L.kmc_query_device(self._h, d_key_hi or None, d_key_lo or None, int(n_keys), d_count or None))

    def profile(self, bases: np.ndarray, offsets: np.ndarray, min_count: int = 1, windows: bool = True, stats: bool = True):
        """Per-read k-mer profile of a host batch against the view (kmc_profile; the batch is not counted):
        (window_count uint32[n_bases] or None, read_stats uint64[n_reads, 5] or None)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = max(int(offsets.shape[0]) - 1, 0)
        win = np.zeros(bases.shape[0], np.uint32) if windows else None
        rs = np.zeros((n_reads, PROFILE_WORDS), np.uint64) if stats else None
        self._chk(self._L.kmc_profile(self._h, bases.ctypes.data, offsets.ctypes.data, n_reads, int(min_count),
                                      win.ctypes.data if windows else None, rs.ctypes.data if stats else None))
        return win, rs

    def profile_device(self, d_bases: int, d_offsets: int, n_reads: int, n_bases: int, min_count: int, d_window_count: int, d_read_stats: int):
        self._chk(self._L.kmc_profile_device(self._h, d_bases or None, d_offsets or None, int(n_reads), int(n_bases), int(min_count),
                                             d_window_count or None, d_read_stats or None))

    def profile_tensors(self, bases, offsets, min_count: int = 1, windows: bool = True, stats: bool = True):
        """torch tensors on this ctx's GPU (bases uint8[n_bases], padded as for add_batch_tensors; offsets int64[n_reads+1]):
        (window_count int32 tensor holding the uint32 bit patterns or None, read_stats int64[n_reads, 5] tensor or None).
        Asynchronous on the ctx stream: call sync() (or order the consumer behind the ctx stream) before reading."""
        import torch
        assert bases.is_cuda and offsets.is_cuda and bases.is_contiguous() and offsets.is_contiguous()
        n_reads, n_bases = max(offsets.numel() - 1, 0), bases.numel()
        win = torch.zeros(n_bases, dtype=torch.int32, device=bases.device) if windows else None
        rs = torch.zeros((n_reads, PROFILE_WORDS), dtype=torch.int64, device=bases.device) if stats else None
        if windows or stats:
            torch.cuda.synchronize(bases.device)  # (the zero fills ran on torch's stream, the profile runs on the ctx's)
        self.profile_device(bases.data_ptr(), offsets.data_ptr(), n_reads, n_bases, min_count,
                            win.data_ptr() if windows and n_bases else 0, rs.data_ptr() if stats and n_reads else 0)
        return win, rs

    # -- multi-GPU reduce, small tables (one fixed-size all-gather; distributed.py) --
    def slab_words(self, slab_entries: int) -> int:
        return int(self._L.kmc_slab_words(self._h, int(slab_entries)))

    def pack_slab_device(self, d_slab: int, slab_entries: int):
        """After finalize(): this table as one fixed-size slab (or an 'oversize' marker)."""
        self._chk(self._L.kmc_pack_slab_device(self._h, d_slab, int(slab_entries)))

    def merge_slabs_device(self, d_slabs: int, n_slabs: int, slab_entries: int, my_part: int, n_parts: int):
        """Add every pair of the gathered slabs that this rank owns; oversize slabs are skipped
        and show up in stats().n_slabs_skipped after the next finalize()."""
        self._chk(self._L.kmc_merge_slabs_device(self._h, d_slabs, int(n_slabs), int(slab_entries), int(my_part), int(n_parts)))

    def poll(self):
        """Synchronise and read the device counters (stats, launch-planner history) without finalizing."""
        self._chk(self._L.kmc_poll(self._h))

    def sync(self):
        """Wait for everything queued on the ctx's stream (no counters are read)."""
        self._chk(self._L.kmc_sync(self._h))

    def forget_source(self, memo: bool = True, history: bool = False):
        self._chk(self._L.kmc_forget_source(self._h, (1 if memo else 0) | (2 if history else 0)))

    def stats(self) -> Stats:
        s = Stats()
        self._chk(self._L.kmc_get_stats(self._h, C.byref(s)))
        return s


def count_file_multi(counters, path: str) -> Tuple[int, int]:
    """One FASTA file on several ctxs of this process (normally one per GPU); counters[0] holds the
    reduced table afterwards."""
    L = lib()
    arr = (C.c_void_p * len(counters))(*[c._h for c in counters])
    nd, nt = C.c_uint64(), C.c_uint64()
    rc = L.kmc_count_file_multi(arr, len(counters), os.fsencode(path), C.byref(nd), C.byref(nt))
    if rc:
        raise KmcError(rc, L.kmc_last_error(counters[0]._h).decode())
    return nd.value, nt.value


def owner_of(key_hi: int, key_lo: int, n_parts: int) -> int:
    return int(lib().kmc_owner_of(int(key_hi), int(key_lo), int(n_parts)))


def encode_key(kmer, canonical: bool = True) -> Tuple[int, int]:
    """(key_hi, key_lo) of an ASCII k-mer of 1..63 upper-case ACGT characters (kmc_encode_key)."""
    b = kmer.encode() if isinstance(kmer, str) else bytes(kmer)
    hi, lo = C.c_uint64(), C.c_uint64()
    rc = lib().kmc_encode_key(b, len(b), 1 if canonical else 0, C.byref(hi), C.byref(lo))
    if rc:
        raise KmcError(rc, lib().kmc_status_string(rc).decode())
    return hi.value, lo.value


def count_file(path: str, k: Optional[int] = None, canonical: bool = True, device: int = 0, algo: int = ALGO_AUTO) -> Table:
    """FASTA path in, sorted table out.  k=None is the reference's own computation (main.rs:58-90)."""
    mode = MODE_LR if k is None else MODE_CONTIG
    with KmerCounter(k=k or 54, canonical=canonical, mode=mode, device=device, algo=algo) as kc:
        kc.count_file(path)
        return kc.export()


# ---------------------------------------------------------------------------------------------
# synthetic input
# ---------------------------------------------------------------------------------------------
def synth_records_for_bytes(s: Synth, file_bytes: int) -> Tuple[int, int]:
    exact = C.c_uint64()
    n = lib().kmc_synth_records_for_bytes(C.byref(s), int(file_bytes), C.byref(exact))
    return int(n), int(exact.value)


def synth_reads_host(s: Synth, first_record: int, n_records: int) -> Tuple[np.ndarray, np.ndarray]:
    bases = np.empty(n_records * s.read_len, np.uint8)
    offsets = np.empty(n_records + 1, np.uint64)
    rc = lib().kmc_synth_reads_host(C.byref(s), first_record, n_records, bases.ctypes.data, offsets.ctypes.data)
    if rc:
        raise KmcError(rc, lib().kmc_status_string(rc).decode())
    return bases, offsets


def synth_reads_device(s: Synth, first_record: int, n_records: int, d_bases: int, d_offsets: int, device: int = 0, stream: int = 0):
    rc = lib().kmc_synth_reads_device(C.byref(s), first_record, n_records, d_bases, d_offsets, device, stream or None)
    if rc:
        raise KmcError(rc, lib().kmc_status_string(rc).decode())


def read_peak_device(d_buf: int, n_bytes: int, device: int = 0, stream: int = 0, shape: int = 0, iters: int = 5) -> Tuple[float, int]:
    """Measured streaming-read rate (kmc_read_peak_device): (ms per launch, xor checksum)."""
    ms, x = C.c_double(), C.c_uint64()
    rc = lib().kmc_read_peak_device(C.c_void_p(d_buf), int(n_bytes), int(device), C.c_void_p(stream), int(shape), int(iters), C.byref(ms), C.byref(x))
    if rc:
        raise KmcError(rc, "kmc_read_peak_device failed")
    return ms.value, x.value


def debug_mem() -> Tuple[int, int, int, int, int]:
    """The library's own allocation counters, process-wide (kmc_debug_mem): live device bytes, live pinned bytes, device
    allocation calls, pinned allocation calls, frees that the runtime refused.  (Bound here, not in lib(): a build loaded
    through KMC_LIB_PATH for an A/B run may be older than the call.)"""
    f = lib().kmc_debug_mem
    f.argtypes, f.restype = [C.POINTER(C.c_uint64 * 5)], None
    out = (C.c_uint64 * 5)()
    f(out)
    return tuple(int(v) for v in out)
