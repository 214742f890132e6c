"""Parameter sweeps without a GPU: the specification (engine/sweep.py), the
state tensors and their contract on CPU tensors, the host seed draws, the
per-group statistics and the CLI flags."""
import json
import os

import numpy as np
import pytest
import torch

from distributed_cluster_gpus_amd.configs.paper import build_arrivals
from distributed_cluster_gpus_amd.engine.sweep import AXES, Sweep, SweepBase
from distributed_cluster_gpus_amd.parallel.sharding import replica_shard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(REPO, "distributed_cluster_gpus_amd", "ops")
needs_ext = pytest.mark.skipif(
    not os.path.exists(os.path.join(OPS, "_sim_hip.so")),
    reason="_sim_hip.so not built")

BASE = SweepBase.of(*build_arrivals(), power_cap=0.0)


# ---------------- specification ----------------
def test_grid_is_the_product_with_the_last_axis_fastest():
    sw = Sweep.grid(inf_rate=[3, 6], power_cap=[0, 30000, 60000])
    assert sw.n_groups == 6 and sw.axes == ("inf_rate", "power_cap")
    pts = [(sw.point(g)["inf_rate"], sw.point(g)["power_cap"])
           for g in range(6)]
    assert pts == [(3, 0), (3, 30000), (3, 60000),
                   (6, 0), (6, 30000), (6, 60000)]
    # axes not named take the base value
    full = sw.resolved(BASE)
    assert full.shape == (6, 7)
    assert (full[:, AXES.index("inf_amp")] == 0.6).all()
    assert (full[:, AXES.index("trn_rate")] == 0.3).all()
    assert full[4].tolist() == [6, 0.6, 300, 0.3, 0.0, 3600.0, 30000]


def test_points_takes_an_explicit_list():
    sw = Sweep.points([{"inf_rate": 3, "inf_amp": 0.6, "trn_rate": 0.3},
                       {"trn_rate": 0.0, "inf_rate": 6},
                       {"inf_rate": 9, "inf_amp": 0.0}])
    assert sw.n_groups == 3
    assert sw.axes == ("inf_rate", "inf_amp", "trn_rate")   # AXES order
    full = sw.resolved(BASE)
    assert full[1].tolist() == [6, 0.6, 300, 0.0, 0.0, 3600.0, 0.0]
    assert full[2, 1] == 0.0 and full[2, 3] == 0.3
    df = sw.frame(BASE)
    assert list(df.columns) == ["group"] + list(AXES) and len(df) == 3
    assert list(sw.frame().columns) == ["group", "inf_rate", "inf_amp",
                                        "trn_rate"]


@pytest.mark.parametrize("axes,reason", [
    (dict(inf_rate=[-1.0]), "rate must be >= 0"),
    (dict(trn_rate=[0.3, -0.1]), "rate must be >= 0"),
    (dict(inf_period=[0.0]), "period must be > 0"),
    (dict(trn_period=[-5.0]), "period must be > 0"),
    (dict(inf_amp=[float("nan")]), "not finite"),
    (dict(inf_rate=[float("inf")]), "not finite"),
    (dict(power_cap=[float("inf")]), "not finite"),
    (dict(size=[1.0]), "unknown sweep axis"),
])
def test_a_bad_value_is_a_value_error(axes, reason):
    with pytest.raises(ValueError, match=reason):
        Sweep.grid(**axes)
    with pytest.raises(ValueError, match=reason):
        Sweep.points([{k: v[-1] for k, v in axes.items()}])


def _validate(sw, **kw):
    args = dict(base=BASE, algo="default_policy", replicas=12,
                arrival_trace=None, arrival_pregen=True, subwave=64)
    args.update(kw)
    sw.validate(**args)


def test_every_configuration_a_sweep_cannot_run_on_is_a_value_error():
    rates = Sweep.grid(inf_rate=[3, 6])
    caps = Sweep.grid(power_cap=[0, 30000])
    _validate(rates)
    _validate(caps, algo="cap_greedy")
    with pytest.raises(ValueError, match="not a multiple"):
        _validate(rates, replicas=13)
    off = SweepBase.of(*build_arrivals(trn_mode="off"))
    with pytest.raises(ValueError, match="trn_rate .*'off'"):
        _validate(Sweep.grid(trn_rate=[0.1, 0.2]), base=off)
    _validate(rates, base=off)          # the other job type may be swept
    for algo in ("cap_uniform", "eco_route", "carbon_cost", "default_policy"):
        with pytest.raises(ValueError, match="power_cap axis needs"):
            _validate(caps, algo=algo)
    with pytest.raises(ValueError, match="chsac_af"):
        _validate(rates, algo="chsac_af")
    with pytest.raises(ValueError, match="arrival_trace"):
        _validate(rates, arrival_trace=(np.zeros((1, 1, 1)),) * 2)
    with pytest.raises(ValueError, match="arrival_pregen=False"):
        _validate(rates, arrival_pregen=False)
    with pytest.raises(ValueError, match="subwave=8"):
        _validate(rates, subwave=8)


def test_the_engine_rejects_them_before_it_looks_for_a_gpu(paper_sc):
    """BatchedEngine validates the sweep first, so these are ValueErrors
    here too, where there is no GPU to construct an engine on."""
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    inf, trn = build_arrivals()
    for kw, reason in (
            (dict(sweep=Sweep.grid(power_cap=[0, 1e4])), "power_cap axis"),
            (dict(sweep=Sweep.grid(inf_rate=[1, 2]), algo="chsac_af"),
             "chsac_af"),
            (dict(sweep=Sweep.grid(inf_rate=[1, 2]), subwave=8), "subwave=8"),
            (dict(sweep=Sweep.grid(inf_rate=[1, 2]), arrival_pregen=False),
             "arrival_pregen=False"),
            (dict(sweep=Sweep.grid(inf_rate=[1, 2, 3]), replicas=16),
             "not a multiple")):
        args = dict(algo="default_policy", replicas=12)
        args.update(kw)
        with pytest.raises(ValueError, match=reason):
            BatchedEngine(paper_sc, inf, trn, **args)


def test_slices_and_table_under_uneven_shards():
    """R = 20, G = 4 (5 per group) over 3 ranks of 7 / 7 / 6 replicas."""
    sw = Sweep.grid(inf_rate=[1.0, 2.0], power_cap=[10.0, 20.0])
    shards = [replica_shard(20, k, 3) for k in range(3)]
    assert [(s.start, s.count) for s in shards] == [(0, 7), (7, 7), (14, 6)]
    assert [sw.slice_of(g, shards[0]) for g in range(4)] == \
        [(0, 5), (5, 7), (7, 7), (7, 7)]
    assert [sw.slice_of(g, shards[1]) for g in range(4)] == \
        [(0, 0), (0, 3), (3, 7), (7, 7)]
    assert [sw.slice_of(g, shards[2]) for g in range(4)] == \
        [(0, 0), (0, 0), (0, 1), (1, 6)]
    # empty slices are empty, and the slices of a shard tile it
    for s in shards:
        cuts = [sw.slice_of(g, s) for g in range(4)]
        assert sum(b - a for a, b in cuts) == s.count
    whole = replica_shard(20, 0, 1)
    arr, cap = sw.table(whole, BASE)
    assert arr.shape == (20, 2, 3) and cap.shape == (20,)
    assert arr.dtype == np.float64 and cap.dtype == np.float64
    assert arr[:, 0, 0].tolist() == [1.0] * 10 + [2.0] * 10
    assert cap.tolist() == ([10.0] * 5 + [20.0] * 5) * 2
    assert (arr[:, 0, 1] == 0.6).all() and (arr[:, 0, 2] == 300.0).all()
    assert (arr[:, 1] == [0.3, 0.0, 3600.0]).all()
    for s in shards:
        a, c = sw.table(s, BASE)
        assert np.array_equal(a, arr[s.start:s.end])
        assert np.array_equal(c, cap[s.start:s.end])
    with pytest.raises(ValueError, match="not a multiple"):
        sw.table(replica_shard(21, 0, 1), BASE)
    with pytest.raises(ValueError, match="group 4"):
        sw.slice_of(4, whole)


# ---------------- state and contract ----------------
R, TCAP, QCAP = 6, 8, 16


def _state(sc, algo, sweep, shard=None):
    from distributed_cluster_gpus_amd.engine.state import (alloc_state,
                                                           engine_cfg,
                                                           engine_dims)
    inf, trn = build_arrivals()
    shard = shard or replica_shard(R, 0, 1)
    dims = engine_dims(sc, algo=algo, n_rep=shard.count, tcap=TCAP,
                       qcap=QCAP, power_cap=45000.0, sweep=sweep,
                       rep_id_offset=shard.start)
    base = SweepBase.of(inf, trn, 45000.0)
    table = sweep.table(shard, base) if sweep is not None else None
    return (alloc_state(dims, sc, "cpu", None, table),
            engine_cfg(dims, sc, inf, trn), dims)


def test_alloc_state_fills_the_sweep_tensors(paper_sc):
    sw = Sweep.grid(inf_rate=[3.0, 9.0], power_cap=[0.0, 30000.0, 60000.0])
    t, cfg, dims = _state(paper_sc, "cap_greedy", sw)
    assert dims.sweep and dims.sweep_cap and cfg["sweep_cap"] == 1
    assert t["sw_arr"].shape == (R, 2, 3) and t["sw_arr"].dtype == torch.float64
    assert t["sw_cap"].shape == (R,) and t["sw_cap"].dtype == torch.float64
    assert t["sw_arr"][:, 0, 0].tolist() == [3.0] * 3 + [9.0] * 3
    assert t["sw_cap"].tolist() == [0.0, 30000.0, 60000.0] * 2
    # a rank's tensors are its rows of the whole table
    sh = replica_shard(R, 1, 2)
    t1, _, _ = _state(paper_sc, "cap_greedy", sw, sh)
    assert torch.equal(t1["sw_arr"], t["sw_arr"][3:])
    assert torch.equal(t1["sw_cap"], t["sw_cap"][3:])
    # no power_cap axis: sw_cap holds the base cap, and nobody reads it
    t2, cfg2, dims2 = _state(paper_sc, "default_policy",
                             Sweep.grid(trn_rate=[0.1, 0.2]))
    assert dims2.sweep and not dims2.sweep_cap and cfg2["sweep_cap"] == 0
    assert t2["sw_cap"].tolist() == [45000.0] * R
    assert t2["sw_arr"][:, 1, 0].tolist() == [0.1] * 3 + [0.2] * 3
    # no sweep: no tensors
    t3, cfg3, dims3 = _state(paper_sc, "default_policy", None)
    assert not dims3.sweep and "sw_arr" not in t3 and "sw_cap" not in t3


def test_engine_dims_rejects_a_sweep_without_the_ring(paper_sc):
    from distributed_cluster_gpus_amd.engine.state import engine_dims
    sw = Sweep.grid(inf_rate=[1, 2])
    for kw in (dict(algo="chsac_af"),
               dict(algo="joint_nf", arrival_pregen=False)):
        with pytest.raises(ValueError, match="arrival-ring generator"):
            engine_dims(paper_sc, n_rep=4, sweep=sw, **kw)
    with pytest.raises(ValueError, match="cap_greedy"):
        engine_dims(paper_sc, n_rep=4, algo="joint_nf",
                    sweep=Sweep.grid(power_cap=[1, 2]))


@needs_ext
def test_the_contract_lists_and_checks_the_sweep_tensors(paper_sc):
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    mod = load_sim_hip("_sim_hip")
    caps = Sweep.grid(power_cap=[0.0, 30000.0])
    t, cfg, _ = _state(paper_sc, "cap_greedy", caps)
    rows = {n: (dt, need) for n, dt, need in
            mod.BatchedSimHip(t, cfg).contract()}
    assert rows["sw_arr"] == ("Double", R * 6)
    assert rows["sw_cap"] == ("Double", R)
    # one wrong shape per tensor, and a wrong dtype, by name
    for field, bad in (("sw_arr", torch.zeros(R, 2, 2, dtype=torch.float64)),
                       ("sw_cap", torch.zeros(R - 1, dtype=torch.float64)),
                       ("sw_arr", t["sw_arr"].to(torch.float32)),
                       ("sw_cap", t["sw_cap"].to(torch.float32))):
        with pytest.raises(ValueError, match=f"'{field}': required .* found "):
            mod.BatchedSimHip(dict(t, **{field: bad}), cfg)
    # without a power_cap axis sw_cap is listed as never dereferenced
    t, cfg, _ = _state(paper_sc, "joint_nf", Sweep.grid(inf_rate=[3.0, 6.0]))
    rows = {n: (dt, need) for n, dt, need in
            mod.BatchedSimHip(t, cfg).contract()}
    assert rows["sw_arr"] == ("Double", R * 6) and rows["sw_cap"][1] == -1
    # the sweep lives in the generator: no ring, no sweep
    with pytest.raises(ValueError, match="'sw_arr'.*arr_cap > 0"):
        mod.BatchedSimHip(t, dict(cfg, arr_cap=0))
    with pytest.raises(ValueError, match="'sw_arr'"):
        load_sim_hip("_sim_hip_mw").BatchedSimHip(t, cfg)


def test_load_tensors_restores_the_sweep_tensors_like_any_tensor(paper_sc):
    from distributed_cluster_gpus_amd.engine.state import load_tensors
    sw = Sweep.grid(inf_rate=[3.0, 6.0])
    t, _, _ = _state(paper_sc, "joint_nf", sw)
    saved = {k: v.clone() for k, v in t.items()}
    t["sw_arr"].zero_()
    load_tensors(t, saved)
    assert torch.equal(t["sw_arr"], saved["sw_arr"])
    plain, _, _ = _state(paper_sc, "joint_nf", None)
    with pytest.raises(ValueError, match="sw_arr"):
        load_tensors(plain, saved)
    with pytest.raises(ValueError, match="sw_arr"):
        load_tensors(t, {k: v for k, v in plain.items()})


# ---------------- seed draws ----------------
def test_seed_arrivals_without_a_sweep_is_what_it_was(paper_sc):
    """(seed 123, 3 replicas): the rows the method returned before it became
    a call to the module-level function, recorded in tests/golden."""
    import types

    from distributed_cluster_gpus_amd.engine.batched import (BatchedEngine,
                                                             seed_arrivals)
    with open(os.path.join(REPO, "tests", "golden",
                           "seed_arrivals_seed123_r3.json")) as f:
        want = np.array([[float.fromhex(x) for x in row]
                         for row in json.load(f)["rows_hex"]])
    inf, trn = build_arrivals()
    shard = replica_shard(3, 0, 1)
    got = seed_arrivals(paper_sc.n_ing, lambda r: (inf, trn), 123, shard)
    assert got.shape == want.shape == (3, paper_sc.n_ing * 2)
    assert np.array_equal(got, want)
    meth = BatchedEngine._seed_arrivals(types.SimpleNamespace(sc=paper_sc),
                                        inf, trn, 123, shard)
    assert np.array_equal(meth, want)


def test_seed_arrivals_of_a_swept_replica_use_its_own_parameters(paper_sc):
    from distributed_cluster_gpus_amd.engine.batched import (BatchedEngine,
                                                             seed_arrivals)
    inf, trn = build_arrivals()
    sw = Sweep.points([
        {"inf_rate": 3, "inf_amp": 0.6, "inf_period": 300, "trn_rate": 0.3},
        {"inf_rate": 6, "inf_amp": 0.3, "inf_period": 120, "trn_rate": 0.0},
        {"inf_rate": 9, "inf_amp": 0.0, "inf_period": 300, "trn_rate": 0.6}])
    whole = replica_shard(6, 0, 1)
    arr, _ = sw.table(whole, SweepBase.of(inf, trn))
    procs = BatchedEngine._sweep_procs(None, inf, trn, arr)
    got = seed_arrivals(paper_sc.n_ing, procs, 7, whole)
    rows = []
    for g in range(3):
        p = sw.point(g)
        u_inf, u_trn = build_arrivals(
            inf_rate=p["inf_rate"], inf_amp=p["inf_amp"],
            inf_period=p["inf_period"], trn_rate=p["trn_rate"])
        # the uniform engine of that point, as shard g of 3
        uni = seed_arrivals(paper_sc.n_ing, lambda r: (u_inf, u_trn), 7,
                            replica_shard(6, g, 3))
        assert np.array_equal(got[2 * g:2 * g + 2], uni)
        rows.append(uni)
    assert not np.array_equal(rows[0], rows[2])
    # a rate of 0 leaves the stream without arrivals
    assert (got[2:4, 1::2] >= 1e300).all() and (got[2:4, 0::2] < 1e300).all()


# ---------------- statistics ----------------
def _values(rng, n):
    v = rng.normal(size=(n, 7)) * [1e6, 50, 40, 2, 0.3, 1, 1e4] + \
        [5e7, 900, 800, 10, 0.5, 3, 2e5]
    v[::4, 4] = np.nan            # replicas without an inference job
    return v


def test_merge_of_a_split_group_is_the_whole_group():
    from distributed_cluster_gpus_amd.analysis.montecarlo import (
        SWEEP_METRICS, SweepStats, merge_sweep_stats)
    rng = np.random.default_rng(5)
    v = _values(rng, 10)          # 2 groups x 5 replicas
    whole = SweepStats.from_values(v, [(0, 5), (5, 10)])
    # each group split 2 / 3 over two parts
    a = SweepStats.from_values(np.concatenate([v[0:2], v[5:7]]),
                               [(0, 2), (2, 4)])
    b = SweepStats.from_values(np.concatenate([v[2:5], v[7:10]]),
                               [(0, 3), (3, 6)])
    m = merge_sweep_stats([a, b])
    assert m.metrics == SWEEP_METRICS == whole.metrics
    assert np.array_equal(m.n, whole.n)
    assert np.array_equal(m.min, whole.min)
    assert np.array_equal(m.max, whole.max)
    np.testing.assert_allclose(m.mean, whole.mean, rtol=1e-12, atol=0)
    np.testing.assert_allclose(m.m2, whole.m2, rtol=1e-12, atol=0)
    # NaN cells are skipped: n counts the replicas that have the figure
    assert whole.n[0].tolist() == [5, 5, 5, 5, 3, 5, 5]
    x = v[5:10, 4]
    x = x[~np.isnan(x)]
    assert whole.mean[1, 4] == pytest.approx(x.mean(), rel=1e-14)
    assert whole.m2[1, 4] == pytest.approx(((x - x.mean()) ** 2).sum(),
                                           rel=1e-12)
    # a part that holds none of a group contributes nothing to it
    c = SweepStats.from_values(v[0:5], [(0, 5), (5, 5)])
    d = SweepStats.from_values(v[5:10], [(0, 0), (0, 5)])
    assert c.n[1].tolist() == [0] * 7 and np.isnan(c.mean[1]).all()
    m = merge_sweep_stats([c, d])
    assert np.array_equal(m.n, whole.n)
    assert np.array_equal(m.mean, whole.mean)
    assert np.array_equal(m.m2, whole.m2)
    rt = SweepStats.from_array(whole.to_array())
    assert np.array_equal(rt.n, whole.n)
    assert np.array_equal(rt.mean, whole.mean, equal_nan=True)


def test_sweep_replica_metrics_and_frame_columns():
    from distributed_cluster_gpus_amd.analysis.montecarlo import (
        SWEEP_METRICS, SWEEP_STAT_COLUMNS, SweepStats, sweep_frame,
        sweep_replica_metrics)
    t = {"energy_j": np.array([[1.0, 2.0], [3.0, 4.0], [0.5, 0.5], [0, 0]]),
         "jobs_done": np.array([4, 2, 1, 0]),
         "jobs_done_inf": np.array([2, 0, 1, 0]),
         "sum_lat": np.array([8.0, 2.0, 3.0, 0.0]),
         "sum_lat_inf": np.array([1.0, 0.0, 0.5, 0.0]),
         "sum_wait": np.array([2.0, 1.0, 0.0, 0.0]),
         "ev_count": np.array([40, 20, 10, 3])}
    v = sweep_replica_metrics(t)
    assert v.shape == (4, len(SWEEP_METRICS))
    assert v[0].tolist() == [3.0, 4, 2, 2.0, 0.5, 0.5, 40]
    assert np.isnan(v[1, 4]) and np.isnan(v[3, 3]) and np.isnan(v[3, 5])
    sw = Sweep.grid(inf_rate=[3.0, 6.0])
    stats = SweepStats.from_values(v, [(0, 2), (2, 4)])
    df = sweep_frame(stats, sw, 0.95, BASE)
    assert list(df.columns) == ["group"] + list(AXES) + [
        f"{m}_{c}" for m in SWEEP_METRICS for c in SWEEP_STAT_COLUMNS]
    assert len(df) == 2 and df["inf_rate"].tolist() == [3.0, 6.0]
    assert df["total_energy_j_mean"].tolist() == [5.0, 0.5]
    assert df["total_energy_j_n"].tolist() == [2, 2]
    se = np.sqrt(((3.0 - 5.0) ** 2 + (7.0 - 5.0) ** 2) / 1) / np.sqrt(2)
    assert df["total_energy_j_stderr"][0] == pytest.approx(se)
    assert df["total_energy_j_ci_hi"][0] == pytest.approx(5.0 + 1.96 * se)
    # one replica with the figure: zero-width interval; none: NaN
    assert df["mean_inf_latency_s_n"].tolist() == [1, 1]
    assert df["mean_inf_latency_s_stderr"].tolist() == [0.0, 0.0]
    assert df["mean_latency_s_n"][1] == 1
    with pytest.raises(ValueError, match="groups"):
        sweep_frame(stats, Sweep.grid(inf_rate=[1, 2, 3]))


def test_group_errors_are_named():
    from distributed_cluster_gpus_amd.engine.batched import raise_on_group_err
    sw = Sweep.grid(inf_rate=[3.0, 6.0, 9.0])
    shard = replica_shard(6, 0, 1)
    raise_on_group_err(np.zeros(6, np.int32), sw, shard)
    with pytest.raises(RuntimeError) as e:
        raise_on_group_err(np.array([0, 0, 0, 0, 1, 5], np.int32), sw, shard)
    msg = str(e.value)
    assert "0x5" in msg and "group 2" in msg and "'inf_rate': 9.0" in msg
    assert "2 of 2 replicas" in msg and "group 0" not in msg


# ---------------- CLI ----------------
def test_cli_sweep_flags():
    import sys
    sys.path.insert(0, REPO)
    import run_sim
    a = run_sim.parse_args(["--engine", "batched"])
    assert run_sim.sweep_axes(a) == {}
    a = run_sim.parse_args(["--engine", "batched", "--sweep-inf-rate",
                            "3,6,9", "--sweep-power-cap", "0,45e3",
                            "--algo", "cap_greedy"])
    axes = run_sim.sweep_axes(a)
    assert axes == {"inf_rate": [3.0, 6.0, 9.0], "power_cap": [0.0, 45000.0]}
    assert list(axes) == ["inf_rate", "power_cap"]
    sw = Sweep.grid(**axes)
    assert sw.n_groups == 6 and sw.point(1) == {"inf_rate": 3.0,
                                                "power_cap": 45000.0}
    a = run_sim.parse_args(["--engine", "batched", "--sweep-trn-rate", "0.1"])
    assert run_sim.sweep_axes(a) == {"trn_rate": [0.1]}
    for bad in (["--sweep-inf-rate", "3,6"],                      # oracle
                ["--engine", "native", "--sweep-power-cap", "1"],
                ["--engine", "batched", "--sweep-inf-rate", "3,x"],
                ["--engine", "batched", "--sweep-trn-rate", ""]):
        with pytest.raises(SystemExit):
            run_sim.parse_args(bad)


def test_sweep_report_writes_one_row_per_point(tmp_path):
    """sweep_report over a stand-in engine (statistics only, no latency
    histograms): population/sweep.csv and the energy-vs-axis figure data"""
    import types

    import pandas as pd

    from distributed_cluster_gpus_amd.analysis.montecarlo import (
        SweepStats, sweep_report)
    sw = Sweep.grid(inf_rate=[3.0, 6.0], power_cap=[1e4, 2e4])
    v = _values(np.random.default_rng(2), 12)
    st = SweepStats.from_values(v, [(3 * g, 3 * g + 3) for g in range(4)])
    eng = types.SimpleNamespace(
        sweep=sw, sweep_base=BASE, sweep_stats=lambda: st,
        dims=types.SimpleNamespace(lat_hist=False),
        shard=replica_shard(12, 0, 1))
    df = sweep_report(eng, str(tmp_path))
    back = pd.read_csv(tmp_path / "population" / "sweep.csv")
    assert list(back.columns) == list(df.columns) and len(back) == 4
    assert back["power_cap"].tolist() == [1e4, 2e4, 1e4, 2e4]
    np.testing.assert_allclose(back["total_energy_j_mean"], st.mean[:, 0])
    fig = pd.read_csv(tmp_path / "population" / "sweep_energy_vs_inf_rate.csv")
    assert {"inf_rate", "mean", "ci_lo", "ci_hi", "point"} <= set(fig.columns)
