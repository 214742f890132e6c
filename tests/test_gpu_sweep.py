"""Parameter sweeps (engine/sweep.py) against uniform engines.

State is replica-major, shards are contiguous and Philox keys use global
replica ids, so group g of a sweep over R replicas is, bit for bit, shard g of
G of a uniform run at that group's parameters.  Every case builds the sweep
engine and G uniform engines (``replicas=R, world=G, rank=g``: the kernels
from before the sweep, on the same global replica ids), gives all of them the
same advance() calls and, after EVERY call, requires every replica-leading
tensor of the sweep engine, sliced to the group, to be torch.equal to the
uniform engine's, and err to be 0.
"""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="needs a ROCm GPU")

SW = {"sw_arr", "sw_cap"}
# (inf rate, amp, period; trn rate)
RATE_POINTS = [(3.0, 0.6, 300.0, 0.3), (6.0, 0.3, 120.0, 0.0),
               (9.0, 0.0, 300.0, 0.6)]
TO_END = [(60, 300)] * 3 + [(61.0, 10 ** 9)]


def _engine(*, arrivals=None, **over):
    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    inf, trn = arrivals or build_arrivals()
    kw = dict(algo="default_policy", duration=60.0, log_interval=5.0,
              out_dir=None, enable_logs=False, seed=123)
    kw.update(over)
    return BatchedEngine(paper_scenario(), inf, trn, **kw)


def _uniform_of(sweep_eng, g, **over):
    """The uniform engine of group g: shard g of G at the group's point."""
    from distributed_cluster_gpus_amd.configs.paper import build_arrivals
    sw = sweep_eng.sweep
    p = sw.point(g, sweep_eng.sweep_base)
    base_inf, base_trn = sweep_eng.arrival_inf, sweep_eng.arrival_trn
    arrivals = build_arrivals(
        inf_mode=base_inf.mode, inf_rate=p["inf_rate"], inf_amp=p["inf_amp"],
        inf_period=p["inf_period"], trn_mode=base_trn.mode,
        trn_rate=p["trn_rate"])
    assert arrivals[1].amp == p["trn_amp"] and \
        arrivals[1].period == p["trn_period"]
    return _engine(arrivals=arrivals, power_cap=p["power_cap"],
                   replicas=sweep_eng.shard.global_replicas,
                   world=sw.n_groups, rank=g, **over)


def _family(sweep, replicas, **over):
    """(sweep engine, its G uniform engines)"""
    eng = _engine(sweep=sweep, replicas=replicas, **over)
    assert eng.sweep is sweep and SW <= set(eng.t)
    unis = [_uniform_of(eng, g, **over) for g in range(sweep.n_groups)]
    for g, u in enumerate(unis):
        assert (u.shard.start, u.shard.end) == eng.sweep.slice_of(g, eng.shard)
        assert not (SW & set(u.t)) and set(u.t) == set(eng.t) - SW
    return eng, unis


def _group_rows(eng, k, a, b, uni_shape):
    """rows [a, b) of a replica-leading tensor; None for any other tensor
    (one whose shape does not depend on the replica count: the uniform engine
    holds fewer replicas and has it in the same shape)"""
    x = eng.t[k]
    if tuple(x.shape) == tuple(uni_shape):
        return None
    if k == "ps_samples":            # replica-minor
        return x[..., a:b]
    assert x.shape[0] == eng.R, k
    return x[a:b]


def _equal(x, y):
    """torch.equal on the bit patterns: an arrival record packs two ints
    into one f64 of its row, a NaN pattern where the kernel routes (dc = -1)"""
    if x.dtype == torch.float64:
        x, y = (z.contiguous().view(torch.int64) for z in (x, y))
    return torch.equal(x, y)


def _same(eng, unis, what):
    torch.cuda.synchronize()
    compared = 0
    for g, u in enumerate(unis):
        a, b = eng.sweep.slice_of(g, eng.shard)
        for k in u.t:
            mine = _group_rows(eng, k, a, b, u.t[k].shape)
            if mine is None:
                continue
            assert mine.shape == u.t[k].shape, (k, mine.shape, u.t[k].shape)
            assert _equal(mine, u.t[k]), f"{what}: group {g}: {k}"
            compared += 1
        assert int(u.t["err"].max()) == 0, what
    assert int(eng.t["err"].max()) == 0, what
    assert compared >= 40 * len(unis)     # the state, not a handful of it


def _calls(eng, unis, calls, what=""):
    for i, (t_target, E) in enumerate(calls):
        for e in [eng] + unis:
            e._sim.advance(float(t_target), E)
        _same(eng, unis, f"{what} call {i} ({t_target}, {E})")


def _all_done(eng):
    return bool((eng.t["done"] == 1).all())


def _rate_sweep():
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    return Sweep.points([dict(inf_rate=r, inf_amp=a, inf_period=p, trn_rate=t)
                         for r, a, p, t in RATE_POINTS])


def _group_sum(eng, k, g):
    a, b = eng.sweep.slice_of(g, eng.shard)
    return eng.t[k][a:b].sum().item()


# ---------------- 1. rates ----------------
@needs_gpu
@pytest.mark.parametrize("algo", ["default_policy", "eco_route", "joint_nf"])
def test_rates(algo):
    """3 groups x 5 replicas: a generator wave (8 replicas) and a block (32)
    hold replicas of different groups and a partly filled tail"""
    eng, unis = _family(_rate_sweep(), 15, algo=algo)
    # the ordinary ring kernels: no power_cap axis
    assert dict((n, need) for n, _, need in eng._sim.contract())["sw_cap"] == -1
    _calls(eng, unis, TO_END, algo)
    assert _all_done(eng) and all(_all_done(u) for u in unis)
    jobs = [_group_sum(eng, "jobs_done", g) for g in range(3)]
    assert len(set(jobs)) == 3 and min(jobs) > 0, jobs


# ---------------- 2. cap ----------------
@needs_gpu
def test_cap():
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    sw = Sweep.grid(power_cap=[0.0, 30000.0, 60000.0, 1e9])
    eng, unis = _family(sw, 12, algo="cap_greedy")
    assert dict((n, need) for n, _, need in eng._sim.contract())["sw_cap"] == 12
    _calls(eng, unis, TO_END, "cap")
    assert _all_done(eng)
    a1, b1 = sw.slice_of(1, eng.shard)
    a3, b3 = sw.slice_of(3, eng.shard)
    assert not torch.equal(eng.t["cur_freq"][a1:b1], eng.t["cur_freq"][a3:b3]) \
        or not torch.equal(eng.t["energy_j"][a1:b1], eng.t["energy_j"][a3:b3])


@needs_gpu
def test_cap_with_rates():
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    sw = Sweep.grid(inf_rate=[3.0, 9.0], power_cap=[30000.0, 60000.0])
    eng, unis = _family(sw, 12, algo="cap_greedy")
    _calls(eng, unis, TO_END, "cap x rates")
    assert _all_done(eng)
    energy = [_group_sum(eng, "energy_j", g) for g in range(4)]
    assert len(set(energy)) == 4, energy


# ---------------- 3. all-base sweep ----------------
@needs_gpu
@pytest.mark.parametrize("algo", ["default_policy", "cap_greedy"])
def test_all_base_sweep_is_the_plain_engine(algo):
    """G = 2 with every point equal to the base: every tensor outside sw_* is
    the plain engine's (cap_greedy: through the swept-cap kernel)"""
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    if algo == "cap_greedy":
        sw, over = Sweep.grid(power_cap=[30000.0, 30000.0]), \
            dict(algo=algo, power_cap=30000.0)
    else:
        sw, over = Sweep.grid(inf_rate=[6.0, 6.0]), dict(algo=algo)
    eng = _engine(sweep=sw, replicas=6, **over)
    plain = _engine(replicas=6, **over)
    assert set(eng.t) - set(plain.t) == SW
    for i, (t_target, E) in enumerate(TO_END):
        eng._sim.advance(float(t_target), E)
        plain._sim.advance(float(t_target), E)
        torch.cuda.synchronize()
        for k in plain.t:
            assert _equal(eng.t[k], plain.t[k]), f"{algo} call {i}: {k}"
        assert int(eng.t["err"].max()) == 0
    assert _all_done(eng) and int(eng.t["jobs_done"].sum()) > 0
    if algo == "cap_greedy":      # the cap was active: the test shows something
        free = _engine(replicas=6, algo=algo, power_cap=0.0)
        free.run()
        assert not torch.equal(free.t["energy_j"], eng.t["energy_j"])


# ---------------- 4. cuts across groups ----------------
@needs_gpu
@pytest.mark.parametrize("algo", ["default_policy", "cap_greedy"])
def test_substeps_and_windows_cut_across_groups(algo):
    """arr_cap = 8: sub-steps of at most 8 events and a wrapping ring; a
    resident capacity of 4 with up to 4 passes: windows that split groups
    (the uniform engines keep their own, single-window plans)"""
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    if algo == "cap_greedy":
        sw = Sweep.grid(inf_rate=[3.0, 9.0], power_cap=[30000.0, 60000.0])
        eng, unis = _family(sw, 12, algo=algo, arr_cap=8)
    else:
        eng, unis = _family(_rate_sweep(), 15, algo=algo, arr_cap=8)
    n = eng.R // eng.sweep.n_groups

    def cuts_groups(plan):
        return any(w[1] < eng.R and (w[0] % n or (w[0] + w[1]) % n)
                   for w in plan)

    # set_launch_plan(4, 4) alone leaves both shapes in one window: the
    # planner's cost model prefers a single launch of 15 replicas on a
    # capacity of 4 (3.6 against 3.75 rounds), and 12 % 4 == 0.  Capacity 7
    # with the planner's costs lowered, as test_gpu_launch_plan.py lowers
    # them, cuts both into 4 passes of windows of 7 replicas.
    eng._sim.set_launch_plan(7, 4, 1, 0)
    plan = eng._sim.launch_plan(100)
    assert max(w[3] for w in plan) <= 8 and cuts_groups(plan)
    _calls(eng, unis, [(60, 100)] * 4, f"{algo} arr_cap 8")
    # ordinary ring: 2048 events a call, in passes of 512
    eng2, unis2 = _family(eng.sweep, eng.shard.global_replicas, algo=algo)
    eng2._sim.set_launch_plan(7, 4, 1, 0)
    assert cuts_groups(eng2._sim.launch_plan(2048))
    _calls(eng2, unis2, [(60, 2048)] * 2 + [(61.0, 10 ** 9)], f"{algo} windows")
    assert _all_done(eng2)
    # and the plan as first proposed, whatever it cuts
    eng3, unis3 = _family(eng.sweep, eng.shard.global_replicas, algo=algo,
                          arr_cap=8)
    eng3._sim.set_launch_plan(4, 4)
    _calls(eng3, unis3, [(60, 100)] * 2, f"{algo} (4, 4)")


# ---------------- 5. quiet group ----------------
@needs_gpu
def test_quiet_group():
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    sw = Sweep.points([dict(inf_rate=6.0, trn_rate=0.3),
                       dict(inf_rate=0.0, trn_rate=0.0),
                       dict(inf_rate=3.0, trn_rate=0.6)])
    eng, unis = _family(sw, 9)
    _calls(eng, unis, TO_END, "quiet")
    a, b = sw.slice_of(1, eng.shard)
    assert int(eng.t["jobs_done"][a:b].sum()) == 0
    assert bool((eng.t["done"][a:b] == 1).all()) and _all_done(eng)
    assert int(eng.t["jobs_done"][:a].min()) > 0


# ---------------- 6. shards ----------------
@needs_gpu
def test_a_shard_of_a_sweep_is_its_rows():
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    sw = Sweep.grid(inf_rate=[3.0, 9.0], power_cap=[30000.0, 60000.0])
    whole = _engine(sweep=sw, replicas=12, algo="cap_greedy")
    part = _engine(sweep=sw, replicas=12, algo="cap_greedy", world=2, rank=1)
    assert (part.shard.start, part.R) == (6, 6)
    assert [sw.slice_of(g, part.shard) for g in range(4)] == \
        [(0, 0), (0, 0), (0, 3), (3, 6)]
    for i, (t_target, E) in enumerate(TO_END):
        whole._sim.advance(float(t_target), E)
        part._sim.advance(float(t_target), E)
        torch.cuda.synchronize()
        n = 0
        for k in part.t:
            if part.t[k].dim() >= 1 and part.t[k].shape[0] == 6 and \
                    whole.t[k].shape[0] == 12:
                assert _equal(whole.t[k][6:12], part.t[k]), \
                    f"call {i}: {k}"
                n += 1
        assert n >= 42 and {"sw_arr", "sw_cap"} <= set(part.t)
        assert int(part.t["err"].max()) == 0


# ---------------- 7. grouped reductions ----------------
def _stats_equal(a, b, fields):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape, f
        assert np.array_equal(x, y, equal_nan=True), f


@needs_gpu
def test_grouped_reductions():
    eng, unis = _family(_rate_sweep(), 15, pop_series=True, latency_hist=True)
    for e in [eng] + unis:
        e.run()
    _same(eng, unis, "run")
    series = ("time", "n", "mean", "m2", "min", "max")
    lat = ("pop_hist", "n", "mean", "m2", "min", "max")
    for g, u in enumerate(unis):
        _stats_equal(eng.population_series(group=g), u.population_series(),
                     series)
        _stats_equal(eng.latency_distribution(group=g),
                     u.latency_distribution(), lat)
    # groups differ, and the ungrouped result is the ensemble's
    assert not np.array_equal(eng.population_series(group=0).mean,
                              eng.population_series(group=2).mean)
    assert int(eng.population_series().n.max()) == 15
    assert int(eng.latency_distribution(group=1).n.max()) == 5
    with pytest.raises(ValueError, match="group 3"):
        eng.population_series(group=3)
    with pytest.raises(RuntimeError, match="without sweep"):
        unis[0].latency_distribution(group=0)


@needs_gpu
def test_ungrouped_reductions_of_an_all_base_sweep_are_the_plain_engines():
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    kw = dict(replicas=6, pop_series=True, latency_hist=True)
    eng = _engine(sweep=Sweep.grid(trn_rate=[0.3, 0.3]), **kw)
    plain = _engine(**kw)
    eng.run()
    plain.run()
    _stats_equal(eng.population_series(group=None), plain.population_series(),
                 ("time", "n", "mean", "m2", "min", "max"))
    _stats_equal(eng.latency_distribution(), plain.latency_distribution(),
                 ("pop_hist", "n", "mean", "m2", "min", "max"))
    # and the per-group statistics are those of the rows
    st = eng.sweep_stats()
    energy = eng.t["energy_j"].sum(dim=1).cpu().numpy()
    assert st.n[:, 0].tolist() == [3, 3]
    assert st.mean[1, 0] == pytest.approx(energy[3:].mean(), rel=1e-14)
    assert st.max[0, 1] == float(eng.t["jobs_done"][:3].max())


# ---------------- 8. checkpoint ----------------
@needs_gpu
def test_checkpoint(tmp_path):
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    sw = Sweep.grid(inf_rate=[3.0, 9.0], power_cap=[30000.0, 60000.0])
    kw = dict(sweep=sw, replicas=8, algo="cap_greedy")
    straight = _engine(**kw)
    first = _engine(**kw)
    for e in (straight, first):
        for t_target, E in TO_END[:2]:
            e._sim.advance(float(t_target), E)
    path = str(tmp_path / "mid.pt")
    first.save_state(path)
    resumed = _engine(**kw)
    resumed.load_state(path)
    for e in (straight, resumed):
        for t_target, E in TO_END[2:]:
            e._sim.advance(float(t_target), E)
    torch.cuda.synchronize()
    for k in straight.t:
        assert _equal(straight.t[k], resumed.t[k]), k
    assert _all_done(resumed) and int(resumed.t["err"].max()) == 0
    other = _engine(sweep=Sweep.grid(inf_rate=[3.0, 8.0],
                                     power_cap=[30000.0, 60000.0]),
                    replicas=8, algo="cap_greedy")
    with pytest.raises(ValueError, match="sw_arr.*differs"):
        other.load_state(path)
    other_cap = _engine(sweep=Sweep.grid(inf_rate=[3.0, 9.0],
                                         power_cap=[30000.0, 50000.0]),
                        replicas=8, algo="cap_greedy")
    with pytest.raises(ValueError, match="sw_cap.*differs"):
        other_cap.load_state(path)
    with pytest.raises(ValueError, match="sw_arr"):
        _engine(replicas=8, algo="cap_greedy").load_state(path)


# ---------------- CLI ----------------
@needs_gpu
def test_cli_writes_the_sweep_report(tmp_path):
    import pandas as pd

    import run_sim
    out = str(tmp_path / "run")
    run_sim.main(["--engine", "batched", "--algo", "cap_greedy",
                  "--replicas", "8", "--duration", "60", "--log-interval", "5",
                  "--log-path", out + os.sep, "--progress", "false",
                  "--latency-hist", "--sweep-inf-rate", "3,9",
                  "--sweep-power-cap", "30000,60000"])
    df = pd.read_csv(os.path.join(out, "population", "sweep.csv"))
    assert len(df) == 4 and df["inf_rate"].tolist() == [3.0, 3.0, 9.0, 9.0]
    assert df["power_cap"].tolist() == [30000.0, 60000.0] * 2
    assert (df["jobs_n"] == 2).all() and (df["jobs_mean"] > 0).all()
    assert df["jobs_mean"][2] > df["jobs_mean"][0]       # thrice the load
    for col in ("inference_p50_s", "inference_p99_s", "inference_p99.9_s",
                "inference_sla_miss_frac"):
        assert col in df.columns and df[col].notna().all(), col
    assert (df["inference_p50_s"] <= df["inference_p99_s"]).all()
    assert df["inference_sla_miss_frac"].between(0.0, 1.0).all()
    # a group without a finished training job has no training figure: on the
    # paper scenario the first training job finishes after about 290 s, so
    # in 60 s every finished job is an inference job
    assert (df["jobs_mean"] == df["jobs_inf_mean"]).all()
    for col in ("training_p99_s", "training_sla_miss_frac"):
        assert col in df.columns and df[col].isna().all(), col
    assert os.path.exists(os.path.join(out, "population",
                                       "sweep_energy_vs_inf_rate.csv"))
