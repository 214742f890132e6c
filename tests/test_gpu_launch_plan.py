"""advance() under a multi-launch plan computes bit for bit what the single
launch computes.

Engine A is pinned to one launch of all replicas (set_launch_plan(0, 1), the
behaviour before the planner); engine B gets a forced resident capacity below
its replica count, so its advance() calls are cut into several launches
(windows) with split event budgets.  Both get identical advance() calls and
are compared with torch.equal: a replica's state is saved and restored
exactly at every event boundary, and a launch that finds a replica at
t_target, at end_time or done leaves it untouched.
"""
import functools
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="needs a ROCm GPU")

EXTRA = ("s_finish", "x_time", "q_len", "done", "err")
PS = ("ps_samples", "ps_tick", "ps_time")


def _names():
    from bench import DUMP_TENSORS
    return tuple(DUMP_TENSORS) + EXTRA


def _make(case="default_policy", replicas=20, subwave=64, **over):
    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    kw = dict(replicas=replicas, duration=60.0, log_interval=5.0,
              out_dir=None, enable_logs=False, subwave=subwave)
    if case == "congested":
        # the congested configuration of test_gpu_wave_select.py
        inf = ArrivalProcess(mode="poisson", rate=30.0)
        trn = ArrivalProcess(mode="poisson", rate=2.0)
        kw.update(algo="debug", seed=11, num_fixed_gpus=8, fixed_freq=0.3,
                  tcap=256)
    else:
        inf, trn = build_arrivals()
        kw.update(algo=case, seed=123)
        if case == "cap_greedy":
            kw.update(power_cap=60000.0)
    kw.update(over)
    return BatchedEngine(sc, inf, trn, **kw)


def _snap(eng, names):
    torch.cuda.synchronize()
    return {n: eng.t[n].detach().cpu().clone() for n in names}


def _assert_same(a, b, what):
    for n in a:
        assert torch.equal(a[n], b[n]), f"{what}: {n}"


def _windows_ok(plan, R, cap, E):
    """several windows, none above the capacity, budgets summing to E"""
    assert len(plan) > 1, plan
    got = [0] * R
    for first, count, split, ev_a, ev_b in plan:
        assert count <= cap
        for s in range(count):
            got[(first + s) % R] += ev_a if s < split else ev_b
    assert got == [E] * R


# ------------------------------------------------------- repeated advances

CALLS = (1, 7, 1000) * 4


@functools.lru_cache(maxsize=None)
def _reference_calls():
    """single-launch states after each call of CALLS (computed once, shared
    and never modified)"""
    eng = _make()
    eng._sim.set_launch_plan(0, 1)
    assert len(eng._sim.launch_plan(1000)) == 1
    out = [_snap(eng, _names())]
    for E in CALLS:
        eng._sim.advance(60.0, E)
        out.append(_snap(eng, _names()))
    return out


# capacity, lowered: with the planner's own constants (a pass of at least 256
# events, a launch costing 32) only E = 1000 is cut; with both lowered to
# (1, 0) E = 7 is cut too, into passes of 2 to 4 events
@needs_gpu
@pytest.mark.parametrize("cap,lowered", [(12, True), (8, True), (14, False),
                                         (19, False)])
def test_repeated_advances(cap, lowered):
    ref = _reference_calls()
    eng = _make()
    if lowered:
        eng._sim.set_launch_plan(cap, 8, min_quantum=1, launch_cost=0)
    else:
        eng._sim.set_launch_plan(cap, 8)
    assert eng._sim.resident_capacity() == cap
    _windows_ok(eng._sim.launch_plan(1000), 20, cap, 1000)
    if lowered:
        _windows_ok(eng._sim.launch_plan(7), 20, cap, 7)
    else:
        assert eng._sim.launch_plan(7) == [(0, 20, 20, 7, 7)]
    assert eng._sim.launch_plan(1) == [(0, 20, 20, 1, 1)]
    exact = 0
    for i, E in enumerate(CALLS):
        eng._sim.advance(60.0, E)
        got = _snap(eng, _names())
        _assert_same(ref[i + 1], got, f"call {i} (E={E})")
        exact += bool((got["ev_count"] - ref[i]["ev_count"] == E).all())
    assert exact >= 1, "no call advanced every replica by exactly E"
    assert int(got["err"].max()) == 0


# ------------------------------------------------------------ huge budget

@needs_gpu
def test_t_target_boundary_under_huge_budget():
    a, b = _make(), _make()
    a._sim.set_launch_plan(0, 1)
    b._sim.set_launch_plan(12, 8)
    _windows_ok(b._sim.launch_plan(10 ** 9), 20, 12, 10 ** 9)
    # every replica stops at t_target inside its first pass; the later
    # passes find it there and must change nothing
    for t_target in (30.0, 60.0):
        a._sim.advance(t_target, 10 ** 9)
        b._sim.advance(t_target, 10 ** 9)
        sa, sb = _snap(a, _names()), _snap(b, _names())
        _assert_same(sa, sb, f"t_target {t_target}")
        if t_target == 30.0:
            assert int(sa["done"].max()) == 0
            assert float(sa["now"].max()) <= 30.0
    assert bool((sb["done"] == 1).all())
    # done replicas: one more call is a no-op on both
    b._sim.advance(60.0, 1000)
    _assert_same(sb, _snap(b, _names()), "advance after done")


# -------------------------------------------------------- other algorithms

def _run_pair(names, cap, lowered=False, **kw):
    a, b = _make(**kw), _make(**kw)
    a._sim.set_launch_plan(0, 1)
    if lowered:
        b._sim.set_launch_plan(cap, 8, min_quantum=1, launch_cost=0)
    else:
        b._sim.set_launch_plan(cap, 8)
    R, E = a.t["done"].numel(), a.events_per_launch
    _windows_ok(b._sim.launch_plan(E), R, cap, E)
    sta, stb = a.run(), b.run()
    sa, sb = _snap(a, names), _snap(b, names)
    _assert_same(sa, sb, str(kw))
    assert bool((sb["done"] == 1).all()) and int(sb["err"].max()) == 0
    assert sta["events"] == stb["events"] > 0
    return a, b


@needs_gpu
@pytest.mark.parametrize("case", ["joint_nf", "cap_greedy", "congested"])
def test_other_algorithms_to_completion(case):
    _run_pair(_names(), 12, case=case, replicas=16, events_per_launch=1000)


@needs_gpu
def test_8_lane_build():
    # 2.5 capacities: cut only with the launch cost lowered
    _run_pair(_names(), 16, lowered=True, replicas=40, subwave=8,
              events_per_launch=1000)


@needs_gpu
def test_population_series():
    a, b = _run_pair(_names() + PS, 12, pop_series=True,
                     events_per_launch=1000)
    assert int(b.t["ps_tick"].min().item()) > 0


# ------------------------------------------------------------ plan choice

@needs_gpu
def test_chsac_is_always_one_launch():
    eng = _make(case="chsac_af", replicas=16, rl_warmup=10 ** 9, seed=3)
    for cap in (0, 5, 12, 15):
        eng._sim.set_launch_plan(cap, 8, min_quantum=1, launch_cost=0)
        assert eng._sim.launch_plan(4000) == [(0, 16, 16, 4000, 4000)]


@needs_gpu
def test_runtime_capacity():
    R, E = 4096, 4000
    eng = _make(replicas=R)
    eng._sim.set_launch_plan(0, 8)
    cap = eng._sim.resident_capacity()
    print("resident capacity (replicas):", cap)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    # whole blocks of 2 replicas on every CU
    assert cap > 0 and cap % (2 * n_cu) == 0
    plan = eng._sim.launch_plan(E)
    if cap >= R or R % cap == 0:
        assert plan == [(0, R, R, E, E)]
    else:
        _windows_ok(plan, R, cap, E)
