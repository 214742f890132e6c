"""Launch planner (ops/csrc/hip/launch_plan.hpp), host side, no GPU.

A small stand-alone program that includes the header is compiled with the
system C++ compiler under -fsanitize=address,undefined and run directly; it
prints every plan of the sweep and the assertions are made here.

The properties hold for every plan; two of them read differently for n = 1.
A single pass IS the single launch of all R replicas, window {0, R, R, E, E},
whatever C is (that is what R % C == 0 must give, and R may exceed C there),
so "windows are at most C" and "L == ceil(R*n/C)" are asserted for n > 1 and
n = 1 is asserted to be exactly that one window.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR_DIR = os.path.join(REPO, "distributed_cluster_gpus_amd", "ops", "csrc",
                       "hip")
MIN_QUANTUM = 256          # PLAN_MIN_QUANTUM, restated: the test is the spec
R_RANGE = range(1, 41)
C_RANGE = range(1, 25)
E_VALUES = (0, 1, 2, 7, 255, 256, 4000, 2 ** 40 + 3)
PASSES = (1, 3, 8)

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "launch_plan.hpp"

static void emit(int R, int C, long long E, int mp) {
  dcg::LaunchPlan p = dcg::make_launch_plan(R, C, E, mp);
  std::printf("P %d %d %lld %d %d %zu\n", R, C, E, mp, p.n_passes,
              p.windows.size());
  for (const dcg::LaunchWindow& w : p.windows)
    std::printf("W %d %d %d %lld %lld\n", w.first, w.count, w.split, w.ev_a,
                w.ev_b);
}

int main(int argc, char** argv) {
  if (argc > 1) {  // one plan: R C E max_passes
    emit(std::atoi(argv[1]), std::atoi(argv[2]), std::atoll(argv[3]),
         std::atoi(argv[4]));
    return 0;
  }
  const long long Es[] = {0, 1, 2, 7, 255, 256, 4000, (1ll << 40) + 3};
  const int mps[] = {1, 3, 8};
  for (int R = 1; R <= 40; ++R)
    for (int C = 1; C <= 24; ++C)
      for (long long E : Es)
        for (int mp : mps) emit(R, C, E, mp);
  std::printf("Q %lld %lld %d\n", dcg::PLAN_MIN_QUANTUM, dcg::PLAN_LAUNCH_COST,
              dcg::PLAN_MAX_PASSES);
  return 0;
}
"""


def _parse(text):
    """{(R, C, E, mp): (n, [windows])} from the driver's output."""
    plans, cur, consts = {}, None, None
    for line in text.splitlines():
        f = line.split()
        if f[0] == "P":
            R, C, E, mp, n, L = map(int, f[1:])
            cur = (n, [], L)
            plans[(R, C, E, mp)] = cur
        elif f[0] == "W":
            cur[1].append(tuple(map(int, f[1:])))
        elif f[0] == "Q":
            consts = tuple(map(int, f[1:]))
    for key, (n, ws, L) in plans.items():
        assert len(ws) == L, key
    return {k: (n, ws) for k, (n, ws, _) in plans.items()}, consts


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("launch_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = str(d / "driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", HDR_DIR, str(src),
                    "-o", exe], check=True)

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], check=True,
                           capture_output=True, text=True)
        assert r.stderr == "", r.stderr   # a sanitizer report
        return _parse(r.stdout)
    return run


@pytest.fixture(scope="module")
def sweep(planner):
    plans, consts = planner()
    assert consts is not None
    return plans, consts


def _check_plan(R, C, E, mp, n, ws):
    assert 1 <= n <= mp
    # replay the launches: slot s of a window serves (first + s) % R
    budgets = [[] for _ in range(R)]
    for (first, count, split, ev_a, ev_b) in ws:
        assert 1 <= count and 0 <= first < R and 0 <= split <= count
        seen = set()
        for s in range(count):
            r = (first + s) % R
            assert r not in seen, "replica twice in one window"
            seen.add(r)
            budgets[r].append(ev_a if s < split else ev_b)
    want = [E // n + (1 if p < E % n else 0) for p in range(n)]
    for r in range(R):
        # launch order is list order: the passes arrive as 0, 1, .., n-1
        assert budgets[r] == want, (r, budgets[r], want)
        assert sum(budgets[r]) == E
    if n == 1:
        assert ws == [(0, R, R, E, E)]
    else:
        assert all(w[1] <= C for w in ws)
        assert len(ws) == -(-R * n // C)
        assert min(want) >= MIN_QUANTUM


def test_sweep_properties(sweep):
    plans, consts = sweep
    assert consts[0] == MIN_QUANTUM
    assert len(plans) == len(R_RANGE) * len(C_RANGE) * len(E_VALUES) * len(PASSES)
    multi = 0
    for (R, C, E, mp), (n, ws) in plans.items():
        _check_plan(R, C, E, mp, n, ws)
        multi += n > 1
        if R <= C or R % C == 0 or mp == 1 or E < 2 * MIN_QUANTUM:
            assert n == 1 and ws == [(0, R, R, E, E)], (R, C, E, mp)
    assert multi > 1000   # the sweep does exercise the multi-launch plans


def test_choice_minimises_the_cost_model(sweep):
    """Among n > 1 the plan minimises L(n) * (E/n + o), smallest n on a tie;
    that best n is taken iff it beats the single launch, which costs
    min(L(1), 0.8 * R/C + 0.6) * E + o.  Exact rational arithmetic."""
    plans, (quantum, cost, _) = sweep
    from fractions import Fraction
    for (R, C, E, mp), (n, ws) in plans.items():
        if R <= C or R % C == 0 or E <= 0:
            continue
        adm = [k for k in range(2, mp + 1) if E // k >= quantum]
        single = min(Fraction(-(-R // C)),
                     Fraction(4 * R + 3 * C, 5 * C)) * E + cost
        want = 1
        if adm:
            def c(k):
                return Fraction(-(-R * k // C) * (E + cost * k), k)
            best = min(adm, key=lambda k: (c(k), k))
            if c(best) < single:
                want = best
        assert n == want, (R, C, E, mp, n, want)


def test_large_ensembles_stay_single(planner):
    """Beyond about 2.7 capacities the single launch's steady state beats
    full lockstep rounds (measured; launch_plan.hpp PLAN_SINGLE_*)."""
    for R in (10240, 16384, 65536):
        plans, _ = planner(R, 3072, 4000, 8)
        assert plans[(R, 3072, 4000, 8)] == (1, [(0, R, R, 4000, 4000)])
    for R in (4096, 5120, 7168):
        plans, _ = planner(R, 3072, 4000, 8)
        assert plans[(R, 3072, 4000, 8)][0] == 3


def test_worked_examples(planner):
    # flagship: 4096 replicas on a capacity of 3072, 4000 events
    plans, _ = planner(4096, 3072, 4000, 8)
    n, ws = plans[(4096, 3072, 4000, 8)]
    assert n == 3
    assert ws == [(0, 3072, 3072, 1334, 1334),
                  (3072, 3072, 1024, 1334, 1333),
                  (2048, 3072, 2048, 1333, 1333),
                  (1024, 3072, 3072, 1333, 1333)]
    _check_plan(4096, 3072, 4000, 8, n, ws)
    # 8192 replicas: 8 launches of 4000/3 against 3 rounds of 4000
    plans, _ = planner(8192, 3072, 4000, 8)
    n, ws = plans[(8192, 3072, 4000, 8)]
    assert n == 3 and len(ws) == 8
    assert all(w[1] == 3072 for w in ws)
    _check_plan(8192, 3072, 4000, 8, n, ws)
    # full rounds and everything-resident stay a single launch
    for R in (3072, 6144, 65536 - 65536 % 3072, 100):
        plans, _ = planner(R, 3072, 4000, 8)
        assert plans[(R, 3072, 4000, 8)] == (1, [(0, R, R, 4000, 4000)])
