"""The bench.py output contract, checked on the committed lines of the last GPU runs (profiles/r03_bench_n1.json and the
N > 1 rehearsal lines next to it): the keys and types the driver and the judge read.  Those lines hold what
`bench.py --full` prints (measured read peak, cpu_baseline, exact full-size check); a plain run prints the same keys with
those figures null or absent.  Below: --dump-outputs, on a host stand-in of a counter ctx."""
import json
import os

from conftest import ROOT


def _line(name):
    return json.load(open(os.path.join(ROOT, "profiles", name)))


def test_committed_bench_line_has_the_contract_keys():
    line = _line("r03_bench_n1.json")
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict),
                     ("roofline", dict), ("cpu_baseline", dict)):
        assert key in line and isinstance(line[key], typ), key
    assert line["vs_baseline"] is None and line["scaling"] == "weak" and line["data"] == "synthetic" and line["higher_is_better"] is True
    assert line["n_gpus"] == 1 and line["steps"] == 20 and line["warmup"] == 5          # the driver's command
    assert "workload" in line["config"] and "model" not in line["config"]
    assert line["config"]["workload"].startswith("10 GB synthetic FASTA") and "seed 2" in line["config"]["workload"] and "k=31" in line["config"]["workload"]
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_step"] / (rf["kernel_ms"] * 1e-3) / 1e9) / rf["achieved"] < 1e-3
    # the nominal peak next to the rate a plain read-only kernel reached over the same bytes in the same run
    assert rf["peak_measured"] > 5000 and abs(rf["frac_of_measured"] - rf["achieved"] / rf["peak_measured"]) < 2e-3
    assert "kmc_read_peak_kernel" in rf["peak_measured_by"]["kernel"]
    # traffic is either absent or says where it comes from (PMC passes are not part of a bench run)
    assert rf["traffic"] is None or ("not measured in this run" in rf["traffic_source"] and 0.9 < rf["traffic"] / rf["algorithmic_bytes_per_step"] < 1.2)
    # value is whole-job throughput: k-mers of all steps / elapsed
    kmers = line["config"]["kmers_per_gpu"] * line["n_gpus"]
    assert abs(line["value"] - kmers / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    cb = line["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb and cb["gpu_bit_exact_on_sample"] is True
    assert line["config"]["exact_full_size_check"]["bit_exact"] is True   # the full-size table against the analytic oracle


def test_n_gt_1_default_is_config_4_strong_with_the_weak_figure_appended():
    for n in (2, 3):
        line = _line("r03_rehearsal_n%d_one_gpu_gloo.json" % n)
        assert line["n_gpus"] == n and line["scaling"] == "strong" and line["cpu_baseline"] is None
        w = line["config"]["workload"]
        assert w.startswith("50 GB synthetic FASTA in total, records split over the ranks") and "seed 3" in w and "k=31" in w and ("%dxMI355X" % n) in w
        assert line["config"]["kmers_all_gpus"] == line["config"]["reduced"]["kmers_all_owners"]      # every k-mer of every rank accounted for
        assert line["config"]["exact_full_size_check"]["bit_exact"] is True
        assert line["config"]["reduce_finalize_every"] == 5 and "every step" in line["config"]["every_step_delivers"]
        assert abs(line["value"] - line["config"]["kmers_all_gpus"] / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
        wk = line["weak_scaling"]
        assert wk["scaling"] == "weak" and wk["workload"].startswith("10 GB synthetic FASTA per GPU") and "seed 2" in wk["workload"]
        assert wk["exact_full_size_check"]["bit_exact"] is True and wk["reduced"]["kmers_all_owners"] == wk["kmers_per_gpu"] * n
        assert abs(wk["value"] - wk["kmers_per_gpu"] * n / (wk["ms_per_step"] * 1e-3)) / wk["value"] < 1e-3


def test_sort_path_line_prices_its_own_pipeline():
    line = _line("r03_bench_n1_pool0_1GB.json")
    sp = line["roofline"]["sort_pipeline"]
    assert line["config"]["algo"] == "sort" and sp["key_units_per_kmer"] == 8 and 0 < sp["frac"] < 1
    n_bases, n_kmers = line["config"]["bases_per_gpu"], line["config"]["kmers_per_gpu"]
    assert sp["model_bytes_per_step"] == (n_bases + 8 * n_kmers) * 8


class _HostTable:
    """Stand-in for a counter ctx whose sorted table lives in host memory (device -1: distributed.device_view reads host
    addresses), enough for bench.dump_outputs."""

    def __init__(self, hi, lo, cnt):
        self.device, self.hi, self.lo, self.cnt = -1, hi, lo, cnt

    def finalize(self):
        return len(self.lo), int(self.cnt.sum())

    def export_device(self):
        return (self.hi.ctypes.data if self.hi is not None else 0), self.lo.ctypes.data, self.cnt.ctypes.data, len(self.lo)


def _table(n, seed, with_hi):
    import numpy as np
    rng = np.random.default_rng(seed)
    lo = np.sort(rng.integers(0, 2**64, n, dtype=np.uint64, endpoint=False))
    hi = rng.integers(0, 2**62, n, dtype=np.uint64) if with_hi else None
    cnt = rng.integers(1, 2**32, n, dtype=np.uint64)
    return hi, lo, cnt


def _load(d, prefix=""):
    import numpy as np
    out = {}
    for name in ("key_hi_upper32", "key_hi_lower32", "key_lo_upper32", "key_lo_lower32", "count", "row", "sizes"):
        a = np.load(os.path.join(d, prefix + name + ".npy"))
        assert a.dtype == np.float64, name
        out[name] = a
    return out


def test_dump_outputs_holds_the_table_exactly(tmp_path):
    """--dump-outputs: float64 files from which every key and count of the table comes back bit for bit."""
    import numpy as np
    import bench
    for with_hi in (False, True):
        hi, lo, cnt = _table(5000, 1, with_hi)
        d = tmp_path / ("hi" if with_hi else "lo")
        bench.dump_outputs(_HostTable(hi, lo, cnt), str(d), prefix="rank0_")
        o = _load(str(d), "rank0_")
        u = lambda a: a.astype(np.uint64)
        assert np.array_equal((u(o["key_lo_upper32"]) << np.uint64(32)) | u(o["key_lo_lower32"]), lo)
        want_hi = hi if with_hi else np.zeros_like(lo)
        assert np.array_equal((u(o["key_hi_upper32"]) << np.uint64(32)) | u(o["key_hi_lower32"]), want_hi)
        assert np.array_equal(u(o["count"]), cnt) and np.array_equal(o["row"], np.arange(5000))
        assert o["sizes"].tolist() == [5000, float(cnt.sum())]


def test_dump_outputs_samples_a_large_table_the_same_way_every_time(tmp_path, monkeypatch):
    import numpy as np
    import bench
    assert 7 * 8 * bench.DUMP_MAX_ROWS + 16 <= 64 * 2**20   # the files stay under 64 MB in all, whatever the table's size
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 300)
    hi, lo, cnt = _table(20000, 2, True)
    got = []
    for i in range(2):
        bench.dump_outputs(_HostTable(hi, lo, cnt), str(tmp_path / str(i)))
        got.append(_load(str(tmp_path / str(i))))
    rows = got[0]["row"].astype(np.int64)
    assert len(rows) == 300 and np.all(np.diff(rows) > 0) and rows[-1] < 20000
    for name in got[0]:
        assert np.array_equal(got[0][name], got[1][name]), name
    assert np.array_equal(got[0]["count"].astype(np.uint64), cnt[rows])
    assert np.array_equal((got[0]["key_lo_upper32"].astype(np.uint64) << np.uint64(32)) | got[0]["key_lo_lower32"].astype(np.uint64), lo[rows])
    assert got[0]["sizes"].tolist() == [20000, float(cnt.sum())]
