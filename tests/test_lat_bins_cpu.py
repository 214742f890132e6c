"""Latency-histogram bin arithmetic (ops/csrc/hip/lat_bins.hpp), host side, no
GPU.

A small stand-alone program that includes the header is compiled with the
system C++ compiler under -fsanitize=address,undefined and run directly; it
reads f64 bit patterns and prints the header's bin, lower and upper edge for
each, then lat_rank over a grid.  The assertions are made here, against a
numpy reference written without the header's formulas: frexp / ldexp
arithmetic instead of bit shifts.
"""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR_DIR = os.path.join(REPO, "distributed_cluster_gpus_amd", "ops", "csrc",
                       "hip")
LO, HI = 2.0 ** -14, 2.0 ** 18      # the bins' span
LAST = 1.875 * 2.0 ** 17            # lower edge of bin 255
QS = (0.5, 0.9, 0.99, 0.999)
NS = (1, 5, 100, 12345)

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include "lat_bins.hpp"

int main() {
  static_assert(dcg::LH_SUB_BITS == 3 && dcg::LH_BINS == 256 &&
                dcg::LH_KEY0 == ((1023 - 14) << 3), "constants");
  uint64_t u;
  while (std::scanf("%" SCNx64, &u) == 1) {
    int b = dcg::lat_bin(dcg::lat_double_of(u));
    std::printf("B %016" PRIx64 " %d %016" PRIx64 " %016" PRIx64 "\n", u, b,
                dcg::lat_bits_of(dcg::lat_bin_lower(b)),
                dcg::lat_bits_of(dcg::lat_bin_upper(b)));
  }
  const double qs[] = {0.5, 0.9, 0.99, 0.999};
  const long long ns[] = {1, 5, 100, 12345};
  for (double q : qs)
    for (long long n : ns)
      std::printf("K %.17g %lld %lld\n", q, n, dcg::lat_rank(q, n));
  return 0;
}
"""


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def unbits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def edge_values():
    inf = math.inf
    out = [0.0, -0.0, -1.0, 5e-324, 1e-310, 2.2250738585072014e-308,
           1e-300, 1e-6, 1e300, inf, -inf, math.nan, 1.0, 0.5, 3.0]
    for v in (LO, HI, LAST, 1.125 * LO, 1.0, 1.125):
        out += [v, np.nextafter(v, -inf), np.nextafter(v, inf)]
    return [float(v) for v in out]


def sweep_values():
    """Log-uniform over the exact range [2^-14, 1.875 * 2^17)."""
    rng = np.random.default_rng(7)
    v = np.exp(rng.uniform(np.log(LO), np.log(LAST), 4000))
    return [float(x) for x in v[(v >= LO) & (v < LAST)]]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("lat_bins")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", HDR_DIR, str(src),
                    "-o", exe], check=True)
    values = edge_values() + sweep_values()
    r = subprocess.run([exe], check=True, capture_output=True, text=True,
                       input="".join(f"{bits(v):016x}\n" for v in values))
    assert r.stderr == "", r.stderr   # a sanitizer report
    lines = r.stdout.splitlines()
    rows = {}
    for f in (l.split() for l in lines if l.startswith("B")):
        rows[int(f[1], 16)] = (int(f[2]), unbits(int(f[3], 16)),
                               unbits(int(f[4], 16)))
    assert len(rows) == len({bits(v) for v in values})
    return rows, [l.split() for l in lines if l.startswith("K")]


def ref_bin(x):
    """Octave and eighth of x by frexp; everything outside clamps."""
    if not x > 0.0:                 # 0, negatives, NaN
        return 0
    if math.isinf(x):
        return 255
    m, e = math.frexp(x)            # x = m * 2^e, 0.5 <= m < 1
    octave, eighth = e - 1, int(math.floor((2.0 * m - 1.0) * 8.0))
    return max(0, min(255, (octave + 14) * 8 + eighth))


def ref_edges(b):
    lo = math.ldexp(1.0 + (b % 8) / 8.0, b // 8 - 14)
    hi = math.ldexp(1.0 + (b % 8 + 1) / 8.0, b // 8 - 14)
    return lo, (hi if b < 255 else math.inf)


def test_bins_of_the_edge_cases(out):
    rows, _ = out
    for v in edge_values():
        b, lo, hi = rows[bits(v)]
        assert b == ref_bin(v), v
        assert (lo, hi) == ref_edges(b), v
    assert rows[bits(0.0)][0] == 0 and rows[bits(5e-324)][0] == 0
    assert rows[bits(float(np.nextafter(LO, 0)))][0] == 0
    assert rows[bits(LO)][0] == 0 and rows[bits(1.125 * LO)][0] == 1
    assert rows[bits(float(np.nextafter(LAST, 0)))][0] == 254
    assert rows[bits(LAST)][0] == 255
    assert rows[bits(float(np.nextafter(HI, 0)))][0] == 255
    assert rows[bits(HI)][0] == 255 and rows[bits(1e300)][0] == 255
    assert rows[bits(LAST)][1:] == (LAST, math.inf)
    assert rows[bits(0.0)][1:] == (LO, 1.125 * LO)


def test_every_bin_brackets_its_samples_within_an_eighth(out):
    rows, _ = out
    sweep = sweep_values()
    assert len(sweep) > 3900
    seen = set()
    for x in sweep:
        b, lo, hi = rows[bits(x)]
        assert b == ref_bin(x) and (lo, hi) == ref_edges(b), x
        assert lo <= x < hi <= 1.125 * x, (x, lo, hi)
        seen.add(b)
    assert min(seen) == 0 and max(seen) == 254 and len(seen) > 250


def test_ranks(out):
    _, ranks = out
    got = {(float(f[1]), int(f[2])): int(f[3]) for f in ranks}
    assert set(got) == {(q, n) for q in QS for n in NS}
    for (q, n), k in got.items():
        assert k == math.ceil(q * float(n)) and 1 <= k <= n
    assert got[(0.5, 5)] == 3 and got[(0.99, 100)] == 99
    assert got[(0.999, 12345)] == 12333 and got[(0.9, 1)] == 1
