"""CPU-side checks of the abundance histogram and count-range filter: the library exports the three entry points and
rejects a NULL ctx, the CLI rejects bad values of its new options before touching a GPU, and the multi-rank histogram
(distributed.global_histogram) sums the owners' spectra over gloo."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, SAMPLE

NEW = ("kmc_histogram", "kmc_filter_device", "kmc_export_filtered")


def test_library_exports_the_spectrum_calls(kmc):
    out = subprocess.run(["nm", "-D", "--defined-only", kmc.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert f" T {s}\n" in out, s
        assert s in kmc.ABI_SYMBOLS
    L = kmc.lib()
    h = np.zeros(16, np.uint64)
    mx = C.c_uint64(7)
    assert L.kmc_histogram(None, 1, 0, 16, h.ctypes.data, C.byref(mx)) == kmc.ERR_ARG
    a, b, c, n, t = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    assert L.kmc_filter_device(None, 2, 0, C.byref(a), C.byref(b), C.byref(c), C.byref(n), C.byref(t)) == kmc.ERR_ARG
    assert L.kmc_export_filtered(None, 2, 0, None, None, None, 0, C.byref(n)) == kmc.ERR_ARG


@pytest.mark.parametrize("argv", [["--min-count", "0"], ["--min-count", "abc"], ["--min-count", "-1"], ["--max-count", "0"],
                                  ["--min-count", "5", "--max-count", "2"], ["--histo", "0"], ["--histo", "16777216"],
                                  ["--histo"], ["-k", "31", "--max-count", "1.5"], ["-k", "31", "--min-count"]])
def test_cli_rejects_bad_spectrum_options(kmc, argv):
    exe = os.path.join(ROOT, "bin", "k-mer-count")
    r = subprocess.run([exe, SAMPLE] + argv, capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout == "" and "k-mer-count:" in r.stderr, (argv, r.returncode, r.stderr)


def test_cli_help_lists_spectrum_options(kmc):
    r = subprocess.run([os.path.join(ROOT, "bin", "k-mer-count"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    for opt in ("--min-count N", "--max-count N", "--histo H"):
        assert opt in r.stderr, opt


def _np_hist(counts, n_bins, lo=1, hi=0):
    c = counts.astype(np.uint64)
    keep = (c >= np.uint64(lo)) & ((c <= np.uint64(hi)) if hi else True)
    return np.bincount(np.minimum(c[keep], np.uint64(n_bins - 1)).astype(np.int64), minlength=n_bins).astype(np.uint64), \
        (int(c[keep].max()) if keep.any() else 0)


class _OwnerStandIn:
    """What distributed.global_histogram needs of a finalized owner ctx: histogram() of the keys it owns."""

    def __init__(self, counts):
        self.counts = counts
        self.device = -1

    def histogram(self, n_bins=10001, min_count=1, max_count=0, return_max=False):
        h, mx = _np_hist(self.counts, n_bins, min_count, max_count)
        return (h, mx) if return_max else h


def _worker_histo(rank, port, world, k, tmpdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        kd = importlib.import_module("k-mer-count_amd.distributed")
        import oracle_py
        bases, offs = oracle_py.parse_fasta(SAMPLE)
        whole = oracle_py.count_kmers(bases, offs, k, True)
        mine = kd.owner_np(whole.key_hi, whole.key_lo, world) == rank     # this rank's owned partition after reduce_tables
        owner = _OwnerStandIn(whole.count[mine])
        out = {}
        for n_bins, lo, hi in ((10001, 1, 0), (50, 1, 0), (2, 1, 0), (40, 2, 100), (131, 7, 7)):
            h, mx = kd.global_histogram(owner, n_bins, lo, hi)
            assert h.dtype == np.uint64 and h.shape == (n_bins,)
            out[f"h_{n_bins}_{lo}_{hi}"] = h
            out[f"m_{n_bins}_{lo}_{hi}"] = np.array([mx], np.uint64)
        np.savez(os.path.join(tmpdir, f"histo{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("k", [21, 63])
def test_world2_global_histogram_equals_whole_table(oracle, tmp_path, k):
    world = 2
    port = 35000 + (os.getpid() + 13 * k) % 2000
    mp.spawn(_worker_histo, args=(port, world, k, str(tmp_path)), nprocs=world, join=True)
    bases, offs = oracle.parse_fasta(SAMPLE)
    whole = oracle.count_kmers(bases, offs, k, True)
    got = [np.load(tmp_path / f"histo{r}.npz") for r in range(world)]
    for n_bins, lo, hi in ((10001, 1, 0), (50, 1, 0), (2, 1, 0), (40, 2, 100), (131, 7, 7)):
        want, want_max = _np_hist(whole.count, n_bins, lo, hi)
        for g in got:   # every rank holds the global result
            assert np.array_equal(g[f"h_{n_bins}_{lo}_{hi}"], want), (n_bins, lo, hi)
            assert int(g[f"m_{n_bins}_{lo}_{hi}"][0]) == want_max
    # the plain spectrum: bincount of the whole table, summing to the distinct keys and (weighted) to the total
    h = got[0]["h_10001_1_0"]
    assert np.array_equal(h, np.bincount(whole.count.astype(np.int64), minlength=10001).astype(np.uint64))
    assert int(h.sum()) == whole.n_distinct and int((h * np.arange(10001, dtype=np.uint64)).sum()) == whole.n_total
