"""Uniform-length batches, host side (k-mer-count_amd/csrc/kmc_walk_uniform.h is plain C++): the closed-form tile geometry
the walk kernel's UNI instantiations use equals what the ragged formulas give from an explicit offsets array i * L, for
every tile and every lane; and the predicate that selects the uniform path accepts exactly the batches it may.

A small stand-alone program is compiled against the header with the host compiler (address + undefined-behaviour
sanitizers when the toolchain links them) and run once; it prints one line per failed check."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HEADER_DIR = os.path.join(ROOT, "k-mer-count_amd", "csrc")

PROGRAM = r"""
#include "kmc_walk_uniform.h"
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } failures++; } } while (0)

int main() {
    const unsigned Ls[] = {1, 15, 16, 17, 33, 150, 400, 401, 416};
    const unsigned long long Ns[] = {1, 63, 64, 65, 129, 1000};
    unsigned long long checked = 0;
    for (unsigned L : Ls) for (unsigned long long n : Ns) {
        std::vector<uint64_t> offs(n + 1);
        for (unsigned long long i = 0; i <= n; ++i) offs[i] = i * L;
        CHECK(kmc_walk_uniform(n, n * L, L), "L=%u n=%llu", L, n);
        const unsigned long long n_tiles = (n + 63) / 64;
        for (unsigned long long t = 0; t < n_tiles; ++t) for (unsigned lane = 0; lane < 64; ++lane) {
            const KmcWalkTile r = kmc_walk_tile_ragged(offs.data(), offs.data() + 1, n, t, lane);
            const KmcWalkTile u = kmc_walk_tile_uniform(n, L, t, lane);
            CHECK(r.have == u.have && r.a == u.a && r.e == u.e && r.A == u.A && r.B == u.B && r.A16 == u.A16 && r.n_pieces == u.n_pieces,
                  "L=%u n=%llu tile=%llu lane=%u: ragged (%u %llu %llu %llu %llu %llu %u) uniform (%u %llu %llu %llu %llu %llu %u)", L, n, t, lane,
                  r.have, (unsigned long long)r.a, (unsigned long long)r.e, (unsigned long long)r.A, (unsigned long long)r.B, (unsigned long long)r.A16, r.n_pieces,
                  u.have, (unsigned long long)u.a, (unsigned long long)u.e, (unsigned long long)u.A, (unsigned long long)u.B, (unsigned long long)u.A16, u.n_pieces);
            // what the closed form is by the issue's own words
            const unsigned long long r0 = 64 * t, nr = n - r0 < 64 ? n - r0 : 64;
            CHECK(u.have == (lane < nr ? 1u : 0u) && u.a == (lane < nr ? (r0 + lane) * L : n * L) && u.e == (lane < nr ? (r0 + lane) * L + L : n * L) &&
                  u.A == r0 * L && u.B == (r0 + nr) * L && u.A16 == (u.A & ~15ull) && u.n_pieces == (unsigned)((u.B - u.A16 + 15) >> 4),
                  "closed form L=%u n=%llu tile=%llu lane=%u", L, n, t, lane);
            checked++;
        }
        // rejected: one base more or less, a larger max_read_len
        CHECK(!kmc_walk_uniform(n, n * L + 1, L), "n*L+1 L=%u n=%llu", L, n);
        CHECK(!kmc_walk_uniform(n, n * L - 1, L), "n*L-1 L=%u n=%llu", L, n);
        CHECK(!kmc_walk_uniform(n, n * L, L + 1), "max_read_len L+1 L=%u n=%llu", L, n);
        CHECK(!kmc_walk_uniform(n, n * L, 416 > L ? 416 : 417), "max_read_len 416 L=%u n=%llu", L, n);
    }
    for (unsigned long long n : Ns) {
        CHECK(!kmc_walk_uniform(n, 0, 0), "L=0 n=%llu", n);
        CHECK(!kmc_walk_uniform(n, n * 417, 417), "L=417 n=%llu", n);
        CHECK(!kmc_walk_uniform(n, n * 1000, 1000), "L=1000 n=%llu", n);
    }
    CHECK(!kmc_walk_uniform(0, 0, 0), "n_reads=0");
    CHECK(!kmc_walk_uniform(0, 0, 400), "n_reads=0 L=400");
    CHECK(!kmc_walk_uniform(0, 400, 400), "n_reads=0 n_bases=400");
    {   // ragged lengths whose sum is a multiple of n_reads, max_read_len their true maximum
        const unsigned lens[][4] = {{100, 200, 300, 200}, {399, 401, 400, 400}, {1, 3, 2, 2}, {0, 416, 208, 208}, {150, 150, 149, 151}};
        for (const auto& v : lens) {
            unsigned long long sum = 0, mx = 0;
            for (unsigned x : v) { sum += x; if (x > mx) mx = x; }
            CHECK(sum % 4 == 0, "test vector");
            CHECK(!kmc_walk_uniform(4, sum, mx), "ragged sum=%llu max=%llu", sum, mx);
        }
    }
    // the division, not a product: n_reads * max_read_len wraps to n_bases here
    CHECK(!kmc_walk_uniform(1ull << 62, 0, 4), "wrapping product");
    CHECK(!kmc_walk_uniform((1ull << 62) + 1, 4, 4), "wrapping product + 4");
    std::printf("checked %llu lanes, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
"""


def _compile(tmp, src, exe):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the host build of libkmc needs it too")
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", HEADER_DIR, src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        r = subprocess.run(base, capture_output=True, text=True)   # (a toolchain without the sanitizer runtimes)
    assert r.returncode == 0, r.stderr[-3000:]


def test_closed_form_geometry_and_predicate(tmp_path):
    src, exe = str(tmp_path / "uni.cpp"), str(tmp_path / "uni")
    with open(src, "w") as f:
        f.write(PROGRAM)
    _compile(tmp_path, src, exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    # every lane of every tile of the 9 x 6 combinations
    want = 9 * sum(((n + 63) // 64) * 64 for n in (1, 63, 64, 65, 129, 1000))
    assert r.stdout.strip().endswith("checked %d lanes, 0 failures" % want), r.stdout[-500:]


def test_header_is_what_the_kernel_includes():
    """The kernel must compute its geometry with the functions tested above, not with a copy."""
    walk = open(os.path.join(HEADER_DIR, "kmc_walk.hip.h")).read()
    api = open(os.path.join(HEADER_DIR, "kmc_api.hip")).read()
    assert '#include "kmc_walk_uniform.h"' in walk
    assert "kmc_walk_tile_uniform(" in walk and "kmc_walk_uniform(" in api
