"""Arrival-ring index arithmetic (ops/csrc/hip/arrival_plan.hpp), host side,
no GPU.

A small stand-alone program that includes the header is compiled with the
system C++ compiler under -fsanitize=address,undefined and run directly; it
prints the header's answers over a sweep and simulates a ring with them.  The
assertions are made here, against a brute-force reference written without the
header's formulas.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR_DIR = os.path.join(REPO, "distributed_cluster_gpus_amd", "ops", "csrc",
                       "hip")
CAPS = (1, 2, 8, 64, 4096)
E_VALUES = (-3, 0, 1, 2, 7, 8, 9, 63, 64, 65, 100, 4095, 4096, 4097, 50000)
HUGE = (4096, 10 ** 9)     # (cap, E): the default ring under a run-to-t_target
BAD_CAPS = (0, -1, 3, 6, 12, 4095, 2 ** 31)

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "arrival_plan.hpp"

int main() {
  const long long caps[] = {1, 2, 8, 64, 4096};
  const long long Es[] = {-3, 0, 1, 2, 7, 8, 9, 63, 64, 65, 100, 4095, 4096,
                          4097, 50000, 1000000000ll};
  for (long long cap : caps)
    for (long long E : Es) {
      if (E == 1000000000ll && cap != 4096) continue;
      int n = dcg::substep_count(E, cap);
      std::printf("S %lld %lld %d", cap, E, n);
      // a huge call has very many sub-steps: print the first and last few
      for (int i = 0; i < n; ++i)
        if (i < 4 || i >= n - 4)
          std::printf(" %d:%lld", i, dcg::substep_budget(E, n, i));
      std::printf(" T %lld\n", dcg::ring_topup_target(E, cap));
    }
  const long long bad[] = {0, -1, 3, 6, 12, 4095, 1ll << 31};
  for (long long c : bad) std::printf("V %lld %d\n", c, dcg::arr_cap_valid(c));
  for (long long c : caps) std::printf("V %lld %d\n", c, dcg::arr_cap_valid(c));
  // a ring driven by the header: push to the target, pop some, many times
  // over; every slot index is printed and checked against a plain queue
  for (int cap : {1, 8, 64}) {
    std::vector<long long> slots(cap, -1);
    int head = 0, count = 0;
    long long next_id = 0, want_id = 0;
    for (int round = 0; round < 40; ++round) {
      long long target = dcg::ring_topup_target(round % 7 + 1, cap);
      while (count < target) {
        int s = dcg::ring_slot(head, count, cap);
        if (s < 0 || s >= cap || slots[s] != -1) { std::printf("R bad\n"); return 1; }
        slots[s] = next_id++;
        ++count;
      }
      int pops = (round * 5 + 3) % (count + 1);
      for (int k = 0; k < pops; ++k) {
        if (slots[head] != want_id) { std::printf("R order\n"); return 1; }
        slots[head] = -1;
        ++want_id;
        head = dcg::ring_slot(head, 1, cap);
        --count;
      }
    }
    std::printf("R %d ok %lld %lld\n", cap, next_id, want_id);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("arrival_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", HDR_DIR, str(src),
                    "-o", exe], check=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert r.stderr == "", r.stderr   # a sanitizer report
    return r.stdout.splitlines()


def _brute_substeps(E, cap):
    """Deal E events one at a time, round robin, over the fewest sub-steps
    that can hold them at `cap` each."""
    if E <= 0:
        return [E]
    n = 1
    while n * cap < E:
        n += 1
    if E > 10 ** 6:                 # dealing one by one would take too long:
        q, rem = divmod(E, n)       # the same deal, in bulk
        return [q + (i < rem) for i in range(n)]
    b = [0] * n
    for k in range(E):
        b[k % n] += 1
    return b


def test_substeps_and_targets(out):
    seen = set()
    for line in out:
        f = line.split()
        if f[0] != "S":
            continue
        cap, E, n = int(f[1]), int(f[2]), int(f[3])
        t_at = f.index("T")
        shown = dict((int(a), int(b)) for a, b in
                     (x.split(":") for x in f[4:t_at]))
        want = _brute_substeps(E, cap)
        assert n == len(want), line
        for i, v in shown.items():
            assert v == want[i], (line, i)
        assert sum(want) == E and max(want) <= max(cap, E if E <= 0 else 0)
        assert all(0 < v <= cap for v in want) or E <= 0
        assert max(want) - min(want) <= 1
        # the ring is topped up to what one sub-step can consume
        assert int(f[t_at + 1]) == max(0, min(E, cap)), line
        seen.add((cap, E))
    assert seen == {(c, e) for c in CAPS for e in E_VALUES} | {HUGE}


def test_capacity_must_be_a_power_of_two(out):
    got = {int(f[1]): int(f[2]) for f in (l.split() for l in out)
           if f[0] == "V"}
    assert got == {**{c: 0 for c in BAD_CAPS}, **{c: 1 for c in CAPS}}


def test_ring_slots_follow_a_plain_queue(out):
    rows = [l.split() for l in out if l.startswith("R")]
    assert [r[1:3] for r in rows] == [["1", "ok"], ["8", "ok"], ["64", "ok"]]
    for r in rows:
        assert int(r[3]) > int(r[1])      # wrapped at least once
