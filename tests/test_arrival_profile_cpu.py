"""Per-ingress arrival rate profiles on the host: the inversion
(models/arrivals.py profile_gap) against exact rational arithmetic, arrival
counts per (ingress, job type, segment), the scalar engines in profile mode
(oracle alone, native against oracle byte for byte), the diurnal builder, the
validation errors of BatchedEngine and Sweep.validate, and the arr_prof part
of the engine's tensor contract."""
import csv
import filecmp
import math
import os
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

import profile_reference as pr
from distributed_cluster_gpus_amd.configs.paper import (paper_scenario,
                                                        single_dc_scenario)
from distributed_cluster_gpus_amd.engine import _philox_host as ph
from distributed_cluster_gpus_amd.models.arrivals import (ArrivalProcess,
                                                          load_profile_csv,
                                                          profile_gap)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(REPO, "distributed_cluster_gpus_amd", "ops")
needs_ext = pytest.mark.skipif(
    not os.path.exists(os.path.join(OPS, "_sim_hip.so")),
    reason="_sim_hip.so not built")


# ------------------------------------------------------- inversion identity

def _identity_error(m, rate, period, t, E):
    """(|Lambda(t, t + g) - E|, tolerance, g)"""
    mm, cum = pr.tables(m)
    g = profile_gap(E, t, rate, period, mm, cum)
    assert g >= 0.0 and math.isfinite(g)
    err = abs(pr.exact_Lambda(t, g, rate, period, m) - Fraction(E))
    return float(err), pr.lambda_tolerance(t, g, rate, period, m), g


@pytest.mark.parametrize("row", pr.EDGE_ROWS, ids=[r[0] for r in pr.EDGE_ROWS])
def test_inversion_identity_edge_cases(row):
    _, m, rate, period, t, E = row
    err, tol, g = _identity_error(m, rate, period, t, E)
    print(f"{row[0]}: g = {g!r}, |Lambda - E| = {err:.3g}, tol = {tol:.3g}")
    assert err <= tol


def test_inversion_identity_random_rows():
    worst = 0.0
    for m, rate, period, t, E in pr.random_rows():
        err, tol, _ = _identity_error(m, rate, period, t, E)
        worst = max(worst, 16.0 * err / tol)
        assert err <= tol, (m, rate, period, t, E)
    print(f"worst |Lambda - E| = {worst:.3g} of 16 units")


def test_gap_is_the_smallest():
    """E = 0 just before a run of zeros stays put; E > 0 there skips the run"""
    m, cum = pr.tables(pr.BASE_TRN)           # (1, 0, 0, 3, 1), 24 s segments
    assert profile_gap(0.0, 10.0, 0.25, 120.0, m, cum) == 0.0
    g = profile_gap(1e-9, 23.999, 0.25, 120.0, m, cum)
    assert g < 1e-6 + 1e-9 / 0.25
    g = profile_gap(0.25 * 0.001 + 1e-9, 23.999, 0.25, 120.0, m, cum)
    assert 48.0 < g < 48.01


@pytest.mark.parametrize("row", pr.OFF_ROWS, ids=[r[0] for r in pr.OFF_ROWS])
def test_off_streams_draw_nothing(row):
    _, m, rate, period, t, E = row
    mm, cum = pr.tables(m)
    assert profile_gap(E, t, rate, period, mm, cum) == ph.D_INF
    assert ph.draw_profile_gap(7, 41, t, rate, period, mm, cum) == \
        (ph.D_INF, 41)

    class NoDraw:
        def expovariate(self, lambd):
            raise AssertionError("an off stream consumed a draw")
    ap = ArrivalProcess(mode="profile", rate=rate, period=period, profile=m)
    assert ap.next_interarrival(t, NoDraw()) == float("inf")


def test_scalar_and_philox_draws_share_the_function():
    ap = ArrivalProcess(mode="profile", rate=1.5, period=120.0,
                        profile=pr.rotations(pr.BASE_INF))
    rng, twin = random.Random(5), random.Random(5)
    for ing in range(8):
        E = twin.expovariate(1.0)
        assert ap.next_interarrival(31.0, rng, ing) == profile_gap(
            E, 31.0, 1.5, 120.0, *pr.tables(ap.profile[ing]))
    key = ph.replica_key(123, 4)
    E = ph.rexp_map(ph.philox_u01(key, 9), 1.0)
    assert ph.draw_profile_gap(key, 9, 31.0, 1.5, 120.0,
                               *pr.tables(pr.BASE_INF)) == (
        profile_gap(E, 31.0, 1.5, 120.0, *pr.tables(pr.BASE_INF)), 10)
    # lambda_t reads the same table
    assert ap.lambda_t(31.0, 0) == 1.5 * 0.5 and ap.lambda_t(31.0, 1) == 0.0
    # the other modes keep their positional form
    assert ArrivalProcess(mode="poisson", rate=2.0).lambda_t(3.0) == 2.0


# ----------------------------------------------------------- counts per cell

def test_counts_per_cell():
    """64 Philox replicas x 8 ingresses x 2 types x 5 segments over 5 cycles:
    every count within 4 standard errors of R * rate * m * seg * cycles,
    zero-rate cells exactly empty"""
    R, NS = 64, 2 * pr.N_ING
    inf, trn = pr.paper_profiles()
    seg = pr.PERIOD / pr.K5
    cycles = pr.DURATION / pr.PERIOD
    counts = np.zeros((pr.N_ING, 2, pr.K5), np.int64)
    for r in range(R):
        key = ph.replica_key(123, r)
        for s in range(NS):
            ap = (inf, trn)[s & 1]
            m, cum = ap._table(s >> 1)
            t, ctr = 0.0, s
            while True:
                g, _ = ph.draw_profile_gap(key, ctr, t, ap.rate, ap.period,
                                           m, cum)
                ctr += NS             # a counter of this stream's own
                t += g
                if t > pr.DURATION:
                    break
                k = min(pr.K5 - 1, int(math.fmod(t, pr.PERIOD) / seg))
                counts[s >> 1, s & 1, k] += 1
    worst = 0.0
    for i in range(pr.N_ING):
        for jt, ap in enumerate((inf, trn)):
            for k in range(pr.K5):
                want = R * ap.rate * ap.profile[i, k] * seg * cycles
                if want == 0:
                    assert counts[i, jt, k] == 0, (i, jt, k)
                    continue
                z = abs(counts[i, jt, k] - want) / math.sqrt(want)
                worst = max(worst, z)
                assert z <= 4.0, (i, jt, k, counts[i, jt, k], want)
    print(f"worst cell: {worst:.2f} standard errors")


# ------------------------------------------------------------ scalar engines

def _job_rows(out):
    with open(os.path.join(out, "job_log.csv"), newline="") as f:
        return list(csv.DictReader(f))


def test_oracle_runs_in_profile_mode(tmp_path):
    """single-DC oracle run: arrivals reconstructed from the job log
    (finish - latency - transfer) per segment within 4 standard errors"""
    from distributed_cluster_gpus_amd.engine.oracle import OracleEngine
    from distributed_cluster_gpus_amd.models.scenario import PAYLOAD_GB
    sc = single_dc_scenario()
    m = (0.0, 0.5, 2.0, 1.0, 1.5)
    rate, period, T_count = 4.0, 60.0, 300.0
    inf = ArrivalProcess(mode="profile", rate=rate, period=period, profile=m)
    trn = ArrivalProcess(mode="off", rate=0.0)
    out = str(tmp_path / "oracle")
    eng = OracleEngine(sc, inf, trn, algo="default_policy",
                       duration=T_count + 60.0, log_interval=5.0, out_dir=out,
                       seed=123, show_progress=False)
    eng.run()
    bw = float(sc.wan_bottleneck_gbps[0][0])      # the oracle's _net_tuple
    transfer = float(sc.wan_latency_s[0][0]) + \
        (PAYLOAD_GB[0] / bw if bw > 0.0 else 0.0)
    seg = period / len(m)
    counts = np.zeros(len(m), np.int64)
    rows = _job_rows(out)
    assert rows
    for r in rows:
        t = float(r["finish_s"]) - float(r["latency_s"]) - transfer
        if t <= T_count:
            counts[min(len(m) - 1, int(math.fmod(max(t, 0.0), period) / seg))] += 1
    for k, mk in enumerate(m):
        want = rate * mk * seg * (T_count / period)
        print(f"segment {k}: {counts[k]} arrivals, expected {want:g}")
        if want == 0:
            assert counts[k] == 0
        else:
            assert abs(counts[k] - want) <= 4.0 * math.sqrt(want)
    assert counts.sum() > 0


@pytest.mark.parametrize("algo", ["default_policy", "joint_nf"])
def test_native_matches_oracle_byte_for_byte(tmp_path, algo):
    from distributed_cluster_gpus_amd.engine.native import NativeEngine
    from distributed_cluster_gpus_amd.engine.oracle import OracleEngine
    inf, trn = pr.paper_profiles(zero_row=3)
    outs = []
    for name, cls, kw in (("oracle", OracleEngine, {"show_progress": False}),
                          ("native", NativeEngine, {})):
        out = str(tmp_path / name)
        cls(paper_scenario(), inf, trn, algo=algo, duration=90.0,
            log_interval=5.0, out_dir=out, seed=7, **kw).run()
        outs.append(out)
    assert len(_job_rows(outs[0])) > 50
    for f in ("job_log.csv", "cluster_log.csv"):
        assert filecmp.cmp(os.path.join(outs[0], f), os.path.join(outs[1], f),
                           shallow=False), f


# ------------------------------------------------------------------- diurnal

def test_diurnal():
    ap = ArrivalProcess.diurnal(6.0, 0.6, 300.0, [0.0, 150.0, 37.0],
                                segments=24)
    assert ap.mode == "profile" and ap.profile.shape == (3, 24)
    for i in range(3):
        _, cum = pr.tables(ap.profile[i])
        assert abs(cum[-1] - 1.0) <= 24 * 2.0 ** -52      # M == 1 to rounding
    # half a period apart: each other's rotation by K / 2
    assert np.allclose(np.roll(ap.profile[0], 12), ap.profile[1],
                       rtol=0, atol=1e-14)
    # the segment means of the sinusoid it stands for
    mid = 1.0 + 0.6 * math.sin(2 * math.pi * (0.5 / 24))
    assert abs(ap.profile[0, 0] - mid) < 0.6 * (2 * math.pi / 24) ** 2 / 24 + 1e-12
    assert ap.profile.min() >= 0.4 - 1e-12 and ap.profile.max() <= 1.6 + 1e-12
    with pytest.raises(ValueError, match="segments = 65"):
        ArrivalProcess.diurnal(6.0, 0.6, 300.0, [0.0], segments=65)


def test_csv_loader(tmp_path):
    p = tmp_path / "prof.csv"
    p.write_text("# two ingresses, three segments\n1, 0, 2.5\n0,0,0\n")
    tab = load_profile_csv(str(p))
    assert tab.tolist() == [[1.0, 0.0, 2.5], [0.0, 0.0, 0.0]]
    ap = ArrivalProcess.from_csv(str(p), rate=2.0, period=90.0)
    assert ap.mode == "profile" and ap.lambda_t(70.0, 0) == 5.0
    p.write_text("1,2\n3\n")
    with pytest.raises(ValueError, match="row lengths"):
        load_profile_csv(str(p))
    p.write_text("1,x\n")
    with pytest.raises(ValueError, match="not a row of numbers"):
        load_profile_csv(str(p))


# --------------------------------------------------------- validation errors

def _prof(profile, **kw):
    return ArrivalProcess(mode="profile", rate=1.5, period=120.0,
                          profile=profile, **kw)


BAD_TABLES = [
    ("negative", [1.0, -0.25, 2.0], r"profile\[0, 1\] = -0\.25 is negative"),
    ("nan", [[1.0, 2.0], [float("nan"), 1.0]], r"profile\[1, 0\] = nan"),
    ("inf", [1.0, float("inf")], r"profile\[0, 1\] = inf is not finite"),
    ("K=0", [], r"K = 0 segments"),
    ("K=65", [1.0] * 65, r"K = 65 segments"),
]


@pytest.mark.parametrize("case", BAD_TABLES, ids=[c[0] for c in BAD_TABLES])
def test_bad_tables_are_rejected_by_value(case, paper_sc):
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    _, table, match = case
    with pytest.raises(ValueError, match=match):
        _prof(table)
    # ... and by the engine, for a process whose table changed after it was
    # built; before the engine looks for a GPU
    ap = _prof([1.0, 2.0])
    ap.profile = table
    with pytest.raises(ValueError, match=match):
        BatchedEngine(paper_sc, ap, ArrivalProcess(mode="poisson", rate=0.3),
                      replicas=4)


def test_row_count_must_be_one_or_n_ing(paper_sc):
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    ap = _prof(np.ones((3, 5)))
    with pytest.raises(ValueError, match=r"3 rows.*n_ing = 8"):
        BatchedEngine(paper_sc, ArrivalProcess(mode="poisson", rate=1.0), ap,
                      replicas=4)
    with pytest.raises(ValueError, match=r"3 rows.*n_ing = 8"):
        ap.profile_rows(8)


ENGINE_CASES = [
    ("chsac_af", dict(algo="chsac_af"), r"algo='chsac_af'"),
    ("subwave=8", dict(subwave=8), r"subwave=8"),
    ("arrival_pregen=False", dict(arrival_pregen=False),
     r"arrival_pregen=False"),
    ("arrival_trace", dict(arrival_trace=(np.ones((4, 16, 2)),
                                          np.ones((4, 16, 2)))),
     r"arrival_trace"),
]


@pytest.mark.parametrize("case", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_engine_paths_that_draw_inline_reject_profile_mode(case, paper_sc):
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    inf, trn = pr.paper_profiles()
    _, kw, match = case
    with pytest.raises(ValueError, match=match) as e:
        BatchedEngine(paper_sc, inf, trn, replicas=4, **kw)
    assert "profile" in str(e.value)
    with pytest.raises(ValueError, match=match):   # one profile type is enough
        BatchedEngine(paper_sc, ArrivalProcess(mode="poisson", rate=1.0), trn,
                      replicas=4, **kw)


def test_sweep_validate():
    from distributed_cluster_gpus_amd.engine.sweep import Sweep, SweepBase
    inf, trn = pr.paper_profiles()
    base = SweepBase.of(inf, ArrivalProcess(mode="sinusoid", rate=0.3, amp=0.5,
                                            period=60.0))
    kw = dict(base=base, algo="default_policy", replicas=24)
    Sweep.grid(inf_rate=[0.75, 1.5, 3.0], inf_period=[60.0, 120.0]).validate(
        **dict(kw, replicas=24))
    Sweep.grid(trn_amp=[0.1, 0.2]).validate(**kw)      # a sinusoid type: fine
    with pytest.raises(ValueError, match=r"inf_amp.*'profile'"):
        Sweep.grid(inf_amp=[0.1, 0.2]).validate(**kw)
    with pytest.raises(ValueError, match=r"inf_amp.*'profile'"):
        Sweep.grid(inf_rate=[1.0, 2.0], inf_amp=[0.1, 0.2]).validate(**kw)


# ------------------------------------------------------------------ contract

R, TCAP, QCAP = 3, 8, 16


def _build(sc, inf, trn, **over):
    from distributed_cluster_gpus_amd.engine.state import (alloc_state,
                                                           engine_cfg,
                                                           engine_dims,
                                                           profile_table)
    dims = engine_dims(sc, algo="default_policy", n_rep=R, tcap=TCAP,
                       qcap=QCAP, log_replica=0, arrivals=(inf, trn), **over)
    tab = profile_table(sc.n_ing, inf, trn) if dims.profile else None
    return (alloc_state(dims, sc, "cpu", prof_table=tab),
            engine_cfg(dims, sc, inf, trn), dims)


def test_profile_table_layout(paper_sc):
    from distributed_cluster_gpus_amd.engine.state import (PROF_SEG, PROF_W,
                                                           profile_table)
    inf, trn = pr.paper_profiles()
    tab = profile_table(8, inf, ArrivalProcess(mode="poisson", rate=0.3))
    assert tab.shape == (16, PROF_W) and PROF_W == 130 and PROF_SEG == 64
    assert not tab[1::2].any()                    # the poisson type's rows
    m, cum = pr.tables(inf.profile[3])
    assert tab[6, 0] == 5 and tuple(tab[6, 1:6]) == m
    assert tuple(tab[6, 65:71]) == cum and not tab[6, 71:].any()
    shared = profile_table(8, _prof([1.0, 3.0]), trn)
    assert (shared[0::2] == shared[0]).all() and shared[0, 0] == 2


def test_state_has_arr_prof_only_in_profile_mode(paper_sc):
    from distributed_cluster_gpus_amd.engine.state import engine_dims
    inf, trn = pr.paper_profiles()
    t, cfg, dims = _build(paper_sc, inf, ArrivalProcess(mode="poisson",
                                                        rate=0.3))
    assert dims.profile and t["arr_prof"].shape == (16, 130)
    assert t["arr_prof"].dtype == torch.float64 and cfg["arr_mode"] == [3, 0]
    sin = ArrivalProcess(mode="sinusoid", rate=6.0, amp=0.6, period=300.0)
    t2, _, dims2 = _build(paper_sc, sin, trn)
    assert dims2.profile and "arr_prof" in t2
    t3, cfg3, dims3 = _build(paper_sc, sin, ArrivalProcess(mode="poisson",
                                                           rate=0.3))
    assert not dims3.profile and "arr_prof" not in t3
    with pytest.raises(ValueError, match="arrival-ring generator"):
        engine_dims(paper_sc, algo="default_policy", n_rep=R,
                    arrivals=(inf, trn), arrival_pregen=False)


@needs_ext
def test_contract_binds_arr_prof(paper_sc):
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    mod = load_sim_hip("_sim_hip")
    inf, trn = pr.paper_profiles()
    t, cfg, dims = _build(paper_sc, inf, trn)
    rows = {n: (dt, need) for n, dt, need in mod.BatchedSimHip(t, cfg).contract()}
    assert rows["arr_prof"] == ("Double", 16 * 130)
    assert t["arr_prof"].numel() == 16 * 130
    # required: a profile-mode engine without it does not bind
    t_missing = {k: v for k, v in t.items() if k != "arr_prof"}
    with pytest.raises(ValueError, match=r"'arr_prof'.*no such tensor"):
        mod.BatchedSimHip(t_missing, cfg)
    # a wrong row width is rejected by name, whatever the element count
    for bad in (torch.zeros((16, 129), dtype=torch.float64),
                torch.zeros((16 * 130,), dtype=torch.float64),
                torch.zeros((130, 16), dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"'arr_prof'.*rows of 130"):
            mod.BatchedSimHip(dict(t, arr_prof=bad), cfg)
    with pytest.raises(ValueError, match=r"'arr_prof'.*Double"):
        mod.BatchedSimHip(dict(t, arr_prof=t["arr_prof"].float()), cfg)
    with pytest.raises(ValueError, match=r"'arr_prof'"):
        mod.BatchedSimHip(dict(t, arr_prof=t["arr_prof"][:15].contiguous()),
                          cfg)
    # not in profile mode: not listed, and a stray table is refused
    sin = ArrivalProcess(mode="sinusoid", rate=6.0, amp=0.6, period=300.0)
    t0, cfg0, _ = _build(paper_sc, sin, ArrivalProcess(mode="poisson",
                                                       rate=0.3))
    names = [n for n, _, _ in mod.BatchedSimHip(t0, cfg0).contract()]
    assert "arr_prof" not in names
    with pytest.raises(ValueError, match=r"'arr_prof'.*no job type"):
        mod.BatchedSimHip(dict(t0, arr_prof=t["arr_prof"]), cfg0)
    # profile mode without the ring has nowhere to run
    t1, cfg1, _ = _build(paper_sc, inf, trn)
    cfg1 = dict(cfg1, arr_cap=0)
    with pytest.raises(ValueError, match=r"'arr_prof'.*arr_cap > 0"):
        mod.BatchedSimHip(t1, cfg1)


# ----------------------------------------------------------------------- CLI

def test_cli_profile_modes(tmp_path):
    import run_sim
    a = run_sim.parse_args(["--inf-mode", "profile", "--ingress-tz-offsets-h",
                            "0,0,6,7,8,8,9,1"])
    assert a.inf_mode == "profile" and len(a.ingress_tz_offsets_h) == 8
    ap = run_sim.profile_arrival("inf", "profile", 6.0, 0.6, 300.0, None,
                                 [0.0, 12.0], 2)
    assert ap.profile.shape == (2, 24)
    assert np.allclose(np.roll(ap.profile[0], 12), ap.profile[1], atol=1e-14)
    with pytest.raises(SystemExit, match="--trn-profile FILE"):
        run_sim.profile_arrival("trn", "profile", 0.3, 0.0, 60.0, None, None, 8)
    with pytest.raises(ValueError, match=r"2 rows.*n_ing = 8"):
        run_sim.profile_arrival("inf", "profile", 6.0, 0.6, 300.0, None,
                                [0.0, 12.0], 8)
    # end to end on both scalar engines, inference from the offsets, training
    # from a file with an ingress that sends no training at all
    csv_path = tmp_path / "trn.csv"
    csv_path.write_text("\n".join(
        "0,0,0" if i == 2 else "1,0.5,1.5" for i in range(8)) + "\n")
    outs = []
    for engine in ("oracle", "native"):
        out = str(tmp_path / engine)
        stats = run_sim.main([
            "--engine", engine, "--duration", "40", "--log-path", out,
            "--progress", "False", "--inf-mode", "profile", "--inf-rate", "2",
            "--inf-period", "40", "--ingress-tz-offsets-h", "0,0,6,7,8,8,9,1",
            "--trn-mode", "profile", "--trn-profile", str(csv_path),
            "--trn-period", "30"])
        assert stats["events"] > 0
        outs.append(out)
    assert filecmp.cmp(os.path.join(outs[0], "job_log.csv"),
                       os.path.join(outs[1], "job_log.csv"), shallow=False)
