"""Pre-generated arrivals (ops/csrc/hip/arrival_ring.hpp) against arrivals
drawn inside the advance kernel.

Every case builds two engines from the same seed, one with the arrival ring
(arrival_pregen=True: pregen_arrivals_kernel fills a per-replica ring, the PRE
advance kernels consume it) and one without (the kernels from before the
ring), gives both the same advance() calls and, after EVERY call, requires
every state tensor outside the ring to be torch.equal and err to be 0.  The
ring changes where the arrival arithmetic runs, never a result: sizes, routes,
arrival times, the Philox counter and everything downstream are bitwise equal.
"""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="needs a ROCm GPU")

RING = {"arr_ring", "arr_head", "arr_count", "gen_arr_next", "gen_ctr",
        "arr_more"}


def _make(pregen, *, algo="default_policy", replicas=6, inf=None, trn=None,
          **over):
    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    d_inf, d_trn = build_arrivals()
    kw = dict(algo=algo, replicas=replicas, duration=60.0, log_interval=5.0,
              out_dir=None, enable_logs=False, seed=123,
              arrival_pregen=pregen)
    kw.update(over)
    return BatchedEngine(paper_scenario(), inf or d_inf, trn or d_trn, **kw)


def _pair(**kw):
    on, off = _make(True, **kw), _make(False, **kw)
    assert on._sim.arrival_pregen() and not off._sim.arrival_pregen()
    assert set(on.t) - set(off.t) == RING and set(off.t) <= set(on.t)
    return on, off


def _same(on, off, what):
    torch.cuda.synchronize()
    for k in off.t:
        assert torch.equal(on.t[k], off.t[k]), f"{what}: {k}"
    assert int(on.t["err"].max()) == 0 and int(off.t["err"].max()) == 0, what


def _calls(on, off, calls, what=""):
    """the same (t_target, max_events) calls on both, compared after each"""
    for i, (t_target, E) in enumerate(calls):
        on._sim.advance(t_target, E)
        off._sim.advance(t_target, E)
        _same(on, off, f"{what} call {i} ({t_target}, {E})")


def _events(eng):
    return int(eng.t["ev_count"].sum().item())


@needs_gpu
def test_wrap_and_substeps():
    """arr_cap = 8: a call of 100 events is 13 sub-steps of 7 or 8 events, and
    the ring wraps many times"""
    on, off = _pair(replicas=5, arr_cap=8)
    plan = on._sim.launch_plan(100)
    assert len(plan) == 13 and sum(w[3] for w in plan) == 100
    assert max(w[3] for w in plan) <= 8
    assert len(off._sim.launch_plan(100)) == 1
    _calls(on, off, [(60.0, 100)] * 6)
    assert _events(on) == 5 * 600


@needs_gpu
@pytest.mark.parametrize("replicas", [1, 70])
def test_tail_lanes(replicas):
    """one replica: a single 8-lane group of a wave is live; 70: three
    blocks of 32 groups, the last one partly filled"""
    on, off = _pair(replicas=replicas)
    _calls(on, off, [(60.0, 300)] * 3)
    assert _events(on) == replicas * 900


@needs_gpu
def test_time_boundary():
    """t_target between two arrivals (about 50 arrivals a second reach a
    replica, so any t_target is), moved on call by call; the huge budgets are
    cut into sub-steps that end as soon as no replica is budget-limited"""
    on, off = _pair()
    _calls(on, off, [(2.0, 10 ** 9), (2.013, 10 ** 9), (2.013, 500),
                     (3.7, 40), (3.7, 10 ** 9), (9.25, 5000)])
    assert float(on.t["now"].max()) <= 9.25
    assert int(on.t["done"].max()) == 0
    # generated ahead of t_target: nothing; the ring holds only what the
    # event budget of call 3 left unconsumed, and now nothing at all
    assert int(on.t["arr_count"].max()) == 0


@needs_gpu
def test_end_of_run():
    """end_time inside the run: the generator's frontier stops at the last
    arrival before it and the counter is the inline engine's"""
    on, off = _pair(duration=8.0, log_interval=2.0)
    for i in range(40):
        _calls(on, off, [(8.0, 700)], f"round {i}")
        if bool((on.t["done"] == 1).all()):
            break
    assert bool((on.t["done"] == 1).all()) and bool((off.t["done"] == 1).all())
    assert int(on.t["arr_count"].max()) == 0
    assert torch.equal(on.t["gen_ctr"], off.t["rng_ctr"])
    assert torch.equal(on.t["gen_arr_next"], off.t["arr_next"])
    _calls(on, off, [(8.0, 700)], "after done")


@needs_gpu
@pytest.mark.parametrize("case", ["inference_off", "poisson_inference_only",
                                  "training_rate_0"])
def test_quiet_streams(case):
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sin = ArrivalProcess(mode="sinusoid", rate=6.0, amp=0.6, period=300.0)
    inf, trn = {
        "inference_off": (ArrivalProcess(mode="off", rate=0.0),
                          ArrivalProcess(mode="poisson", rate=2.0)),
        "poisson_inference_only": (ArrivalProcess(mode="poisson", rate=6.0),
                                   ArrivalProcess(mode="off", rate=0.0)),
        "training_rate_0": (sin, ArrivalProcess(mode="poisson", rate=0.0)),
    }[case]
    on, off = _pair(inf=inf, trn=trn)
    _calls(on, off, [(60.0, 250)] * 3)
    assert _events(on) > 0


@needs_gpu
@pytest.mark.parametrize("cap", [2, 4])
def test_forced_windows(cap):
    """6 replicas under set_launch_plan(cap, 8, 1, 0).  A capacity of 2
    divides 6, so the planner keeps one full launch; a capacity of 4 cuts
    every sub-step into three windows, the middle one with two budgets"""
    on, off = _pair(replicas=6)
    for eng in (on, off):
        eng._sim.set_launch_plan(cap, 8, 1, 0)
    plan = on._sim.launch_plan(300)
    if cap == 2:
        assert plan == [(0, 6, 6, 300, 300)]
    else:
        assert len(plan) == 3 and any(w[2] < w[1] for w in plan)
        assert all(w[1] <= cap for w in plan)
    _calls(on, off, [(60.0, 300)] * 3)
    assert _events(on) == 6 * 900


@needs_gpu
def test_checkpoint_with_a_non_empty_ring(tmp_path):
    on, off = _pair(arr_cap=256)
    _calls(on, off, [(60.0, 200)] * 2)
    assert int(on.t["arr_count"].min()) > 0      # records left in the ring
    path = str(tmp_path / "mid.pt")
    on.save_state(path)
    resumed = _make(True, arr_cap=256)
    resumed.load_state(path)
    for i in range(3):
        _calls(on, off, [(60.0, 200)], f"after save {i}")
        resumed._sim.advance(60.0, 200)
        torch.cuda.synchronize()
        for k in on.t:                            # the ring too
            assert torch.equal(resumed.t[k], on.t[k]), (i, k)


@needs_gpu
def test_population_series():
    on, off = _pair(pop_series=True)
    assert "ps_samples" in off.t
    _calls(on, off, [(60.0, 1500)] * 3)
    assert int(on.t["ps_tick"].min()) > 0


@needs_gpu
@pytest.mark.parametrize("algo,over", [
    ("default_policy", {}), ("bandit", {}), ("eco_route", {}),
    ("cap_greedy", {"power_cap": 60000.0})])
def test_algorithms(algo, over):
    on, off = _pair(algo=algo, replicas=8, **over)
    _calls(on, off, [(60.0, 1200)] * 3)
    assert _events(on) == 8 * 3600
    if algo == "eco_route":                       # the kernel routes itself
        written = on.t["arr_ring"][..., 1] > 0    # t_next of a record
        dc = on.t["arr_ring"].view(torch.int32)[..., 7]
        assert bool(written.any()) and bool((dc[written] == -1).all())


@needs_gpu
def test_applicability():
    """chsac_af and trace mode draw as before whatever is asked; so does the
    8-lane build"""
    eng = _make(True, subwave=8)
    assert not eng._sim.arrival_pregen() and not RING & set(eng.t)
    eng = _make(True, algo="chsac_af", rl_warmup=10 ** 9)
    assert not eng._sim.arrival_pregen() and not RING & set(eng.t)
    with pytest.raises(ValueError, match="power of two"):
        _make(True, arr_cap=100)
