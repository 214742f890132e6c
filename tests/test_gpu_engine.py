"""MI355X batched-engine GPU tests (SURVEY §4 strategies (c)/(d)):
distributional equivalence vs the scalar engines, deterministic-decision
exactness (grid-search / debug pins), conservation checks, contract checks.
All marked gpu — run via gpurun on a real MI355X."""
import csv
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="needs MI355X")


def make_engine(algo="default_policy", replicas=128, duration=120.0,
                out_dir=None, enable_logs=False, **kw):
    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    sc = paper_scenario()
    inf, trn = build_arrivals()
    return BatchedEngine(sc, inf, trn, algo=algo, replicas=replicas,
                         duration=duration, log_interval=5.0, out_dir=out_dir,
                         seed=123, enable_logs=enable_logs, **kw)


def native_population(algo, duration, seeds, **kw):
    """Run the C++ scalar engine over several seeds; return per-seed stats."""
    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.native import NativeEngine
    import tempfile
    rows = []
    for s in seeds:
        sc = paper_scenario()
        inf, trn = build_arrivals()
        with tempfile.TemporaryDirectory() as td:
            eng = NativeEngine(sc, inf, trn, algo=algo, duration=duration,
                               log_interval=5.0, out_dir=td, seed=s, **kw)
            st = eng.run()
        rows.append(st)
    return rows


@needs_gpu
def test_engine_runs_and_conserves():
    eng = make_engine(replicas=256, duration=120.0)
    st = eng.run()
    assert st["events"] > 0
    assert st["jobs_completed"] > 0
    assert int(eng.t["err"].max().item()) == 0
    # utilization integrals positive; busy never negative
    assert int(eng.t["busy"].min().item()) >= 0
    assert float(eng.t["energy_j"].min().item()) > 0  # sleep floor > 0
    # every replica processed a similar order of events (same workload)
    evs = eng.t["ev_count"].cpu().numpy()
    assert evs.min() > 0.5 * evs.mean()
    assert math.isfinite(st["mean_wait_s"]) and st["mean_wait_s"] >= 0.0


@needs_gpu
def test_queueing_delay_metric_positive_under_congestion():
    """sum_wait measures real queueing delay: a config that saturates DCs
    (every job pinned to 8 GPUs, heavy arrivals) must report positive mean
    wait, and an uncongested one ~zero."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    inf = ArrivalProcess(mode="poisson", rate=30.0)
    trn = ArrivalProcess(mode="poisson", rate=2.0)
    eng = BatchedEngine(sc, inf, trn, algo="debug", replicas=16,
                        duration=120.0, log_interval=5.0, out_dir=None,
                        seed=11, enable_logs=False, num_fixed_gpus=8,
                        fixed_freq=0.3, tcap=256)
    st = eng.run()
    assert st["mean_wait_s"] > 0.0, "no wait recorded under congestion"
    inf2 = ArrivalProcess(mode="poisson", rate=0.2)
    trn2 = ArrivalProcess(mode="off", rate=0.0)
    eng2 = BatchedEngine(sc, inf2, trn2, algo="default_policy", replicas=16,
                         duration=120.0, log_interval=5.0, out_dir=None,
                         seed=11, enable_logs=False)
    st2 = eng2.run()
    assert st2["mean_wait_s"] < st["mean_wait_s"]


@needs_gpu
def test_distributional_match_vs_native_default_policy():
    """GPU replica-population means must match the scalar C++ engine's
    cross-seed distribution on total energy, completed jobs and mean latency
    (batched-vs-scalar equivalence, distributional form)."""
    duration = 120.0
    nat = native_population("default_policy", duration, seeds=range(10))
    nat_energy = np.array([r["total_energy_j"] for r in nat])
    nat_jobs = np.array([r["jobs_completed"] for r in nat])

    eng = make_engine(replicas=256, duration=duration)
    st = eng.run()
    gpu_energy = eng.t["energy_j"].sum(dim=1).cpu().numpy()
    gpu_jobs = eng.t["jobs_done"].cpu().numpy().astype(float)

    # population means within 3 combined standard errors
    for g, n, name in ((gpu_energy, nat_energy, "energy"),
                       (gpu_jobs, nat_jobs, "jobs")):
        se = math.sqrt(n.std() ** 2 / len(n) + g.std() ** 2 / len(g))
        assert abs(g.mean() - n.mean()) < 4 * se + 1e-9, \
            f"{name}: gpu {g.mean():.4g} vs native {n.mean():.4g} (se {se:.3g})"


@needs_gpu
def test_distributional_match_joint_nf():
    duration = 100.0
    nat = native_population("joint_nf", duration, seeds=range(8))
    nat_energy = np.array([r["total_energy_j"] for r in nat])
    eng = make_engine(algo="joint_nf", replicas=192, duration=duration)
    eng.run()
    gpu_energy = eng.t["energy_j"].sum(dim=1).cpu().numpy()
    se = math.sqrt(nat_energy.std() ** 2 / len(nat_energy) +
                   gpu_energy.std() ** 2 / len(gpu_energy))
    assert abs(gpu_energy.mean() - nat_energy.mean()) < 4 * se + 1e-9


@needs_gpu
def test_joint_nf_decisions_exact(tmp_path):
    """joint_nf's (n, f) choice is deterministic per (dc, jtype): the GPU
    grid-argmin must equal the CPU best_nf_grid exactly (when not clamped by
    free-GPU pressure)."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.models.coeffs import LatencyCoeffs, PowerCoeffs
    from distributed_cluster_gpus_amd.policies.gridsearch import best_nf_grid
    out = str(tmp_path / "jn")
    eng = make_engine(algo="joint_nf", replicas=8, duration=60.0,
                      out_dir=out, enable_logs=True)
    eng.run()
    sc = paper_scenario()
    expect = {}
    for d, dc in enumerate(sc.dc_names):
        for j, jt in enumerate(("inference", "training")):
            pC = PowerCoeffs(*sc.power_coeffs[d, j, :])
            tC = LatencyCoeffs(*sc.latency_coeffs[d, j, :])
            n, f, *_ = best_nf_grid(8, list(sc.freq_levels), pC, tC,
                                    objective="energy")
            expect[(dc, jt)] = (n, f)
    with open(os.path.join(out, "job_log.csv")) as fh:
        rows = list(csv.DictReader(fh))
    assert rows, "logging replica produced no job rows"
    checked = 0
    for r in rows:
        n_exp, f_exp = expect[(r["dc"], r["type"])]
        # n may be clamped down under GPU pressure; f must match exactly then
        if int(r["n_gpus"]) == n_exp:
            assert abs(float(r["f_used"]) - f_exp) < 1e-9
            checked += 1
    assert checked > len(rows) * 0.5


@needs_gpu
def test_debug_pins_nf(tmp_path):
    """Directly-admitted jobs use the pinned (n, f); queued jobs drain
    through the heuristic (reference behaviour, :922-927) — use a light load
    so nothing queues."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    inf = ArrivalProcess(mode="poisson", rate=0.5)
    trn = ArrivalProcess(mode="off", rate=0.0)
    out = str(tmp_path / "dbg")
    eng = BatchedEngine(sc, inf, trn, algo="debug", replicas=4, duration=90.0,
                        log_interval=5.0, out_dir=out, enable_logs=True,
                        seed=123, num_fixed_gpus=2, fixed_freq=0.7)
    eng.run()
    with open(os.path.join(out, "job_log.csv")) as fh:
        rows = list(csv.DictReader(fh))
    assert rows
    for r in rows:
        assert r["n_gpus"] == "2"
        assert r["f_used"] == "0.700"


@needs_gpu
def test_log_schema_matches_scalar(tmp_path):
    """The batched engine's CSV outputs use the exact reference schemas."""
    from distributed_cluster_gpus_amd.utils.csvlog import (CLUSTER_COLUMNS,
                                                           JOB_COLUMNS)
    out = str(tmp_path / "logs")
    eng = make_engine(replicas=4, duration=40.0, out_dir=out, enable_logs=True)
    eng.run()
    with open(os.path.join(out, "cluster_log.csv")) as fh:
        header = fh.readline().strip().split(",")
    assert header == CLUSTER_COLUMNS
    with open(os.path.join(out, "job_log.csv")) as fh:
        header = fh.readline().strip().split(",")
    assert header == JOB_COLUMNS
    # util/energy sanity on logged rows
    with open(os.path.join(out, "cluster_log.csv")) as fh:
        for row in csv.DictReader(fh):
            assert 0.0 <= float(row["util_inst"]) <= 1.0
            assert 0.0 <= float(row["util_avg"]) <= 1.0001
            assert float(row["power_W"]) > 0


@needs_gpu
def test_bandit_and_eco_route_run():
    for algo in ("bandit", "eco_route", "carbon_cost", "cap_greedy"):
        eng = make_engine(algo=algo, replicas=64, duration=60.0,
                          power_cap=30000.0 if algo == "cap_greedy" else 0.0)
        st = eng.run()
        assert st["jobs_completed"] > 0, algo


@needs_gpu
def test_cap_greedy_reduces_power():
    e1 = make_engine(algo="cap_greedy", replicas=64, duration=100.0,
                     power_cap=0.0)
    e1.run()
    e2 = make_engine(algo="cap_greedy", replicas=64, duration=100.0,
                     power_cap=30000.0)
    e2.run()
    assert float(e2.t["energy_j"].sum().item()) < float(e1.t["energy_j"].sum().item())


@needs_gpu
def test_replica_shard_rng_independent_of_world():
    """Sharding must not change per-replica streams: replica k of a 2-'rank'
    split equals replica k of the single-rank run (same global ids)."""
    e_full = make_engine(replicas=8, duration=60.0)
    e_full.run()
    e_lo = make_engine(replicas=8, duration=60.0, rank=0, world=2)
    e_lo.run()
    e_hi = make_engine(replicas=8, duration=60.0, rank=1, world=2)
    e_hi.run()
    full_jobs = e_full.t["jobs_done"].cpu()
    lo = e_lo.t["jobs_done"].cpu()
    hi = e_hi.t["jobs_done"].cpu()
    assert torch.equal(full_jobs[:4], lo)
    assert torch.equal(full_jobs[4:], hi)
    assert torch.allclose(e_full.t["energy_j"].sum(dim=1).cpu()[:4],
                          e_lo.t["energy_j"].sum(dim=1).cpu())


@needs_gpu
def test_smoke_entry():
    sys.path.insert(0, REPO)
    import __graft_entry__ as ge
    ge.smoke()


@needs_gpu
def test_bench_contract():
    """bench.py default invocation must emit the driver's JSON contract."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        "--steps", "3", "--warmup", "1",
                        "--replicas-per-gpu", "512", "--events-per-step", "200",
                        "--with-rl", "0"],
                       capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
              "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config"):
        assert k in out, k
    assert out["value"] > 0 and out["n_gpus"] == 1
    assert out["metric"] == "sim_events_per_sec"


@needs_gpu
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's per-replica state as
    float64 .npy; --steps sets the timed step count; two runs with the same
    arguments see identical inputs and so produce identical arrays; a plain
    run leaves the --full metrics out."""
    R, E, K, W = 512, 200, 3, 1
    outs = []
    for tag in ("a", "b"):
        d = str(tmp_path / tag)
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                            "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                            "--replicas-per-gpu", str(R),
                            "--events-per-step", str(E), "--dump-outputs", d],
                           capture_output=True, text=True, timeout=300, cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
        res = json.loads(line)
        assert res["steps"] == K and res["ms_per_step"] > 0
        # value is events / elapsed and ms_per_step is elapsed / steps
        assert res["value"] * res["ms_per_step"] * 1e-3 * K == \
            pytest.approx(R * E * K, rel=1e-9)
        assert res["config"]["rl_train_steps_per_sec"] is None
        assert res["config"]["rl_loop_events_per_sec"] is None
        outs.append({f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))})
    a, b = outs
    assert set(a) == set(b) and {"ev_count.npy", "energy_j.npy", "now.npy",
                                 "jobs_done.npy", "sum_lat.npy"} <= set(a)
    for f in a:
        assert a[f].dtype == np.float64 and a[f].shape[0] == R, f
        assert np.array_equal(a[f], b[f]), f"{f} differs between runs"
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    # every replica ran exactly (warmup + steps) launches of E events
    assert (a["ev_count.npy"] == E * (K + W)).all()
    assert (a["energy_j.npy"].sum(axis=1) > 0).all()
    assert (a["jobs_done.npy"] > 0).all()


@needs_gpu
def test_chsac_batched_runs_and_trains(tmp_path):
    """CHSAC-AF on the batched engine: replicas pause at decision points, the
    host serves batched policy actions, transitions flow into replay, SAC
    trains on-device (BASELINE.json config 4 capability)."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    inf = ArrivalProcess(mode="poisson", rate=2.0)
    trn = ArrivalProcess(mode="poisson", rate=0.3)
    out = str(tmp_path / "rl")
    eng = BatchedEngine(sc, inf, trn, algo="chsac_af", replicas=32,
                        duration=120.0, log_interval=5.0, out_dir=out,
                        seed=7, enable_logs=True,
                        rl_warmup=64, rl_batch=32, rl_train_interval=16,
                        events_per_launch=5000)
    st = eng.run()
    assert st["jobs_completed"] > 0
    assert eng.replay.size > 0, "no transitions reached the replay ring"
    assert eng.rl_updates > 0, "SAC never trained"
    assert int(eng.t["err"].max().item()) == 0
    # transitions carry sane rewards/costs
    b = eng.replay.sample(16)
    assert torch.isfinite(b["r"]).all()
    assert (b["costs"]["latency_p99"] >= 0).all()
    assert (b["costs"]["gpu_over"] >= 0).all()
    # logging replica produced job rows
    with open(os.path.join(out, "job_log.csv")) as fh:
        rows = list(csv.DictReader(fh))
    assert rows


@needs_gpu
def test_chsac_batched_respects_masks():
    """Actions applied must come from the masked policy: every served action
    picks a DC its mask allowed, and every device-built DC mask agrees with
    the engine's live free-GPU state at selection time (checked by
    intercepting the serve call, not just by absence of error flags)."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    inf = ArrivalProcess(mode="off", rate=0.0)
    trn = ArrivalProcess(mode="poisson", rate=1.0)
    eng = BatchedEngine(sc, inf, trn, algo="chsac_af", replicas=16,
                        duration=60.0, log_interval=5.0, out_dir=None,
                        seed=3, enable_logs=False, rl_warmup=10**9,
                        events_per_launch=5000, rl_serve="host")
    eng._mfma_serve = False  # route serving through the interceptable torch path
    checked = {"n": 0}
    inner = eng.rl.select_action_batch

    def checking_select(obs, m_dc, m_g, deterministic=False):
        t = eng.t
        pend = (t["req_flag"] == 1).nonzero(as_tuple=True)[0]
        # device-built mask vs live engine state: DC valid <=> free GPUs > 0
        free = (t["total_gpus"].unsqueeze(0) - t["busy"][pend]) > 0
        expect = free.clone()
        expect[(~free).all(dim=1)] = True  # host all-false guard opens mask
        assert torch.equal(m_dc, expect), "DC mask != live free-GPU state"
        a = inner(obs, m_dc, m_g, deterministic=deterministic)
        assert bool(m_dc.gather(1, a["dc"].view(-1, 1)).all()), \
            "served action chose a masked-out DC"
        checked["n"] += int(pend.numel())
        return a

    eng.rl.select_action_batch = checking_select
    st = eng.run()
    assert st["events"] > 0
    assert checked["n"] > 0, "no serve calls intercepted"
    assert int(eng.t["err"].max().item()) == 0


@needs_gpu
def test_state_invariants_and_checkpoint(tmp_path):
    """validate_state cross-checks cached busy/n_running/min-finish against
    first principles (the engine's race/corruption detector), and
    save_state/load_state resumes a run exactly."""
    eng = make_engine(replicas=64, duration=200.0)
    # advance partway
    eng._sim.advance(100.0, 10**9)
    torch.cuda.synchronize()
    assert eng.validate_state()
    ckpt = str(tmp_path / "engine_state.pt")
    eng.save_state(ckpt)
    ev_mid = eng.t["ev_count"].clone()
    # run A continues to the end
    st_a = eng.run()
    jobs_a = eng.t["jobs_done"].clone()
    energy_a = eng.t["energy_j"].clone()
    # run B: fresh engine, restore the checkpoint, continue
    eng2 = make_engine(replicas=64, duration=200.0)
    eng2.load_state(ckpt)
    assert torch.equal(eng2.t["ev_count"], ev_mid)
    st_b = eng2.run()
    assert torch.equal(eng2.t["jobs_done"].cpu(), jobs_a.cpu())
    assert torch.allclose(eng2.t["energy_j"].cpu(), energy_a.cpu())
    assert eng2.validate_state()


@needs_gpu
def test_chsac_batched_via_cli(tmp_path):
    """run_sim.py --engine batched --algo chsac_af end-to-end."""
    out = str(tmp_path / "rl_cli")
    r = subprocess.run([sys.executable, os.path.join(REPO, "run_sim.py"),
                        "--algo", "chsac_af", "--engine", "batched",
                        "--replicas", "16", "--duration", "60",
                        "--inf-mode", "poisson", "--inf-rate", "1.0",
                        "--trn-rate", "0.2", "--upgr-warmup", "50",
                        "--upgr-batch", "32",
                        "--log-path", out, "--progress", "False"],
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.exists(os.path.join(out, "job_log.csv"))
    # RL observability: SAC losses/alpha reach project.log at INFO on the
    # batched production path (round-1 VERDICT item 7)
    with open(os.path.join(out, "project.log")) as fh:
        log_text = fh.read()
    assert "loss_critic" in log_text, "no SAC stats in project.log"


@needs_gpu
@pytest.mark.parametrize("algo,kw,use_own_routing", [
    ("eco_route", {}, True),           # deterministic routing: GPU routes itself
    ("default_policy", {}, False),     # random routing: replay recorded DCs
    ("joint_nf", {}, False),
    ("bandit", {}, False),
    ("cap_greedy", {"power_cap": 0.0}, False),
    # ACTIVE cap: the GPU controller now implements the reference's exact
    # sorted-snapshot atom pass (frozen-rho selection walk, insertion-order
    # tie-break via s_seq, reference reschedule arithmetic), so trajectory
    # parity holds while atoms are being applied every tick
    ("cap_greedy", {"power_cap": 60000.0}, False),
    # cap_uniform with an active cap is a verified no-op (its delta-P probe
    # reads per-job f_used, insensitive to DC-level f; oracle module
    # docstring) — parity proves the GPU treats it identically
    ("cap_uniform", {"power_cap": 60000.0}, False),
    ("debug", {"num_fixed_gpus": 2, "fixed_freq": 0.7}, False),
])
def test_single_replica_exact_trajectory_parity(tmp_path, algo, kw,
                                                use_own_routing):
    """SURVEY §4 (c), exact form: one GPU replica fed the ORACLE's recorded
    arrival stream (+ routed DCs for random-routing algorithms) must
    reproduce the scalar trajectory event-for-event — identical job log
    (jid/dc/n/f/times) and matching cluster-log energy/util columns
    (fp-accumulation tolerance only)."""
    from distributed_cluster_gpus_amd.configs.paper import build_arrivals, paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.engine.oracle import OracleEngine

    duration = 90.0
    sc = paper_scenario()
    inf, trn = build_arrivals()
    rec = []
    out_o = str(tmp_path / "oracle")
    OracleEngine(sc, inf, trn, algo=algo, duration=duration,
                 log_interval=5.0, out_dir=out_o, seed=123,
                 arrival_recorder=rec, **kw).run()
    # build the [1][NS][cap] trace (times, sizes, routed DCs)
    ing_idx = {n: i for i, n in enumerate(sc.ingress_names)}
    dc_idx = {n: i for i, n in enumerate(sc.dc_names)}
    NS = sc.n_ing * 2
    streams = [[] for _ in range(NS)]
    for (tt, ing, jtype, size, dc) in rec:
        s_id = ing_idx[ing] * 2 + (0 if jtype == "inference" else 1)
        streams[s_id].append((tt, size, dc))
    cap = max(len(x) for x in streams) + 1
    times = np.full((1, NS, cap), 1e300)
    sizes = np.zeros((1, NS, cap), np.float64)
    dcs = np.full((1, NS, cap), -1, np.int8)
    for s_id, entries in enumerate(streams):
        for k, (tt, size, dc) in enumerate(entries):
            times[0, s_id, k] = tt
            sizes[0, s_id, k] = size
            if not use_own_routing and dc is not None:
                dcs[0, s_id, k] = dc_idx[dc]

    sc2 = paper_scenario()
    out_g = str(tmp_path / "gpu")
    eng = BatchedEngine(sc2, inf, trn, algo=algo, replicas=1,
                        duration=duration, log_interval=5.0, out_dir=out_g,
                        seed=999,  # RNG unused in replay mode
                        enable_logs=True,
                        arrival_trace=(times, sizes, dcs), **kw)
    eng.run()

    import pandas as pd
    jo = pd.read_csv(os.path.join(out_o, "job_log.csv"))
    jg = pd.read_csv(os.path.join(out_g, "job_log.csv"))
    assert len(jo) == len(jg), f"job count {len(jo)} vs {len(jg)}"
    jo = jo.sort_values("jid").reset_index(drop=True)
    jg = jg.sort_values("jid").reset_index(drop=True)
    for col in ("jid", "ingress", "type", "dc", "n_gpus"):
        assert (jo[col] == jg[col]).all(), f"column {col} diverged"
    # sizes, frequencies and times are f64 end-to-end on the GPU, so event
    # times equal the oracle's up to the rounding of the FMA-contracted device
    # models (tests/test_gpu_models.py); job columns must match to print
    # precision
    for col, tol in (("size", 1e-9), ("f_used", 1e-12), ("net_lat_s", 1e-6),
                     ("start_s", 1e-9), ("finish_s", 1e-9), ("latency_s", 1e-9),
                     ("T_pred", 1e-9), ("P_pred", 1e-9), ("E_pred", 1e-9)):
        d = (jo[col] - jg[col]).abs().max()
        assert d <= tol, f"column {col} max diff {d}"
    co = pd.read_csv(os.path.join(out_o, "cluster_log.csv"))
    cg = pd.read_csv(os.path.join(out_g, "cluster_log.csv"))
    assert len(co) == len(cg)
    key = ["time_s", "dc"]
    m = co.merge(cg, on=key, suffixes=("_o", "_g"))
    assert len(m) == len(co)
    for col in ("busy", "free", "run_total", "run_inf", "run_train",
                "q_inf", "q_train"):
        assert (m[f"{col}_o"] == m[f"{col}_g"]).all(), f"cluster {col} diverged"
    # power/energy use an incremental active-power cache on the GPU vs the
    # oracle's per-event recomputation: identical modulo f64 accumulation
    # order, which can straddle a CSV print-rounding boundary — allow one
    # print quantum plus the fp-accumulation relative tolerance
    for col, quantum, rtol in (("power_W", 0.01, 1e-8),
                               ("energy_kJ", 1e-4, 1e-8),
                               ("util_inst", 1e-4, 1e-12),
                               ("util_avg", 1e-4, 1e-10),
                               ("acc_job_unit", 1e-4, 1e-6),
                               ("freq", 0.0, 1e-12)):
        a, b = m[f"{col}_o"], m[f"{col}_g"]
        d = ((a - b).abs() - (1.01 * quantum + rtol * a.abs())).max()
        assert d <= 0, f"cluster {col} beyond print+fp tolerance by {d}"


@needs_gpu
def test_subwave_variants_bit_identical():
    """The 8-replicas-per-wave engine (subwave=8) must produce bit-identical
    trajectories to the default wave-per-replica engine — same Philox streams,
    same f64 math, different lane geometry."""
    e64 = make_engine(replicas=64, duration=90.0)
    e64.run()
    e8 = make_engine(replicas=64, duration=90.0, subwave=8)
    e8.run()
    for key in ("ev_count", "jobs_done", "jobs_done_inf"):
        assert torch.equal(e64.t[key].cpu(), e8.t[key].cpu()), key
    assert torch.equal(e64.t["energy_j"].cpu(), e8.t["energy_j"].cpu())
    assert torch.equal(e64.t["sum_lat"].cpu(), e8.t["sum_lat"].cpu())


@needs_gpu
def test_chsac_elastic_scaling_on_gpu(tmp_path):
    """Elastic scaling on the batched engine: training completions with other
    training jobs running trigger preempt-all + RL reallocation; preempt
    counts surface in the job log and invariants hold (GPU capability parity
    with the oracle's elastic path)."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    inf = ArrivalProcess(mode="off", rate=0.0)
    trn = ArrivalProcess(mode="poisson", rate=0.5)
    out = str(tmp_path / "el")
    eng = BatchedEngine(sc, inf, trn, algo="chsac_af", replicas=16,
                        duration=1500.0, log_interval=10.0, out_dir=out,
                        seed=5, enable_logs=True, elastic_scaling=True,
                        rl_warmup=10**9,  # act-only, no training needed here
                        events_per_launch=20000)
    st = eng.run()
    assert int(eng.t["err"].max().item()) == 0
    assert st["jobs_completed"] > 0
    assert eng.validate_state()
    with open(os.path.join(out, "job_log.csv")) as fh:
        rows = list(csv.DictReader(fh))
    assert rows
    total_preempts = sum(int(r["preempt_count"]) for r in rows)
    assert total_preempts > 0, "elastic scaling never preempted"
    # preempted jobs keep their identity and complete exactly once
    jids = [r["jid"] for r in rows]
    assert len(jids) == len(set(jids))


@needs_gpu
def test_population_report(tmp_path):
    """Monte-Carlo population statistics over the replica ensemble."""
    from distributed_cluster_gpus_amd.analysis.montecarlo import (
        population_frame, population_report)
    eng = make_engine(replicas=128, duration=90.0)
    eng.run()
    df = population_frame(eng)
    assert len(df) == 128
    rep = population_report(eng, out_dir=str(tmp_path / "pop"))
    e = rep["total_energy_kJ"]
    assert e["std"] > 0 and e["ci_lo"] < e["mean"] < e["ci_hi"]
    assert e["p01"] <= e["p50"] <= e["p99"]
    assert os.path.exists(os.path.join(str(tmp_path / "pop"), "population.csv"))
    assert os.path.exists(os.path.join(str(tmp_path / "pop"),
                                       "population_stats.csv"))


@needs_gpu
def test_train_rl_dp_driver_single_gpu(tmp_path):
    """scripts/train_rl_dp.py end-to-end on one GPU (the 8-GPU DP path minus
    the collectives, which the gloo tests pin)."""
    ckpt = str(tmp_path / "dp.pt")
    r = subprocess.run([sys.executable,
                        os.path.join(REPO, "scripts", "train_rl_dp.py"),
                        "--replicas-per-gpu", "48", "--duration", "150",
                        "--warmup", "100", "--batch", "64",
                        "--train-interval", "64", "--checkpoint", ckpt,
                        "--replay-npz", str(tmp_path / "ds.npz")],
                       capture_output=True, text=True, timeout=900, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["jobs_completed"] > 0 and out["rl_updates"] > 0
    assert os.path.exists(ckpt)
    # offline dataset round-trips into the offline trainer
    from distributed_cluster_gpus_amd.rl.offline import train_offline
    agent, stats = train_offline(str(tmp_path / "ds.npz"), epochs=1,
                                 batch_size=64, device="cuda",
                                 constraints={"latency_p99": 500.0})
    assert stats and np.isfinite(stats[-1]["loss_critic"])


@needs_gpu
def test_rccl_collectives_smoke():
    """Every DP collective code path executes at least once on REAL RCCL
    (world_size=1 communicator on one MI355X): metric all-reduce, fused flat
    gradient all-reduce inside a SAC train step, CMDP cost reduction, and the
    per-launch dp_sync_step control word (round-1 VERDICT item 2: be
    8-GPU-ready; world>1 runs are the driver's to launch)."""
    import torch.distributed as dist
    from distributed_cluster_gpus_amd.parallel.dist import (
        allreduce_tensor_sum, dp_sync_step)
    from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,
                                                       CHSACAgentConfig)
    from distributed_cluster_gpus_amd.rl.replay import ReplayRing
    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29871",
                            world_size=1, rank=0)
    try:
        dev = torch.device("cuda", 0)
        # metric reduction over RCCL
        t = torch.arange(8, dtype=torch.float64, device=dev)
        out = allreduce_tensor_sum(t.clone())
        assert torch.equal(out, t)
        # control-word sync over RCCL
        assert dp_sync_step(0, False, 123, 7) == (0, False, 123, 7)
        # DP SAC train step: fused flat gradient all-reduce + cost reduction
        torch.manual_seed(0)
        agent = CHSACAgent(CHSACAgentConfig(
            obs_dim=49, n_dc=8, n_g_choices=8,
            constraints={"latency_p99": 500.0}, device="cuda"))
        agent.enable_ddp()
        ring = ReplayRing(capacity=512, obs_dim=49, n_costs=1,
                          cost_names=["latency_p99"], n_dc=8, n_g=8,
                          device="cuda", seed=0)
        B = 512
        ring.add_batch(s=torch.randn(B, 49), s_next=torch.randn(B, 49),
                       a_dc=torch.randint(0, 8, (B,)),
                       a_g=torch.randint(0, 8, (B,)),
                       r=torch.randn(B), costs=torch.rand(B, 1) * 100,
                       done=torch.ones(B))
        stats = agent.train_step(ring.sample(256), compute_stats=True)
        assert np.isfinite(stats["loss_critic"])
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()


@needs_gpu
def test_device_actor_forward_matches_torch():
    """The in-kernel actor forward (ops rl_forward_debug — the same device
    math the serve_device path runs) must match the torch actor's logits on
    random obs within fp32 accumulation tolerance."""
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,
                                                       CHSACAgentConfig)
    mod = load_sim_hip()
    torch.manual_seed(11)
    obs_dim, n_dc, n_g, H = 49, 8, 8, 256
    agent = CHSACAgent(CHSACAgentConfig(
        obs_dim=obs_dim, n_dc=n_dc, n_g_choices=n_g,
        constraints={"latency_p99": 500.0}, device="cuda"))
    # flat buffer with the engine's layout
    segs = []
    enc = agent.encoder.net
    for lin in (enc[0], enc[2], enc[4], agent.actor.head_dc[0],
                agent.actor.head_dc[2], agent.actor.head_g[0],
                agent.actor.head_g[2]):
        segs.append(lin.weight.detach().t().contiguous().reshape(-1))
        segs.append(lin.bias.detach().reshape(-1))
    pw = torch.cat(segs).float().cuda()
    obs = torch.randn(256, obs_dim, device="cuda") * 100.0
    out_dc, out_g = mod.rl_forward_debug(pw, obs, H, n_dc, n_g)
    with torch.no_grad():
        ref_dc, ref_g = agent.actor(agent.encoder(obs))
    for got, ref in ((out_dc, ref_dc), (out_g, ref_g)):
        diff = (got - ref).abs().max().item()
        scale = ref.abs().max().item() + 1.0
        assert diff <= 2e-4 * scale, f"logit mismatch {diff} (scale {scale})"


@needs_gpu
def test_chsac_device_serving_runs_and_trains():
    """serve_device end-to-end: the actor runs inside the advance kernel,
    transitions stream out, SAC trains, weights refresh — and throughput per
    launch is far beyond the pause/resume path's one-event-per-pause."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    inf = ArrivalProcess(mode="poisson", rate=2.0)
    trn = ArrivalProcess(mode="poisson", rate=0.3)
    eng = BatchedEngine(sc, inf, trn, algo="chsac_af", replicas=64,
                        duration=200.0, log_interval=5.0, out_dir=None,
                        seed=7, enable_logs=False,
                        rl_warmup=256, rl_batch=64, rl_train_interval=64,
                        events_per_launch=50000)
    assert eng._serve_device
    st = eng.run()
    assert st["jobs_completed"] > 0
    assert eng.replay.size > 0
    assert eng.rl_updates > 0, "SAC never trained in device-serve mode"
    assert int(eng.t["err"].max().item()) == 0
    b = eng.replay.sample(32)
    assert torch.isfinite(b["r"]).all()
    assert (b["costs"]["latency_p99"] >= 0).all()
    eng.validate_state()
    # device mode must finish in FAR fewer launches than events processed
    # (pause/resume needed ~one launch per decision)
    assert eng.timing["launches"] * 100 < st["events"]


@needs_gpu
def test_chsac_device_vs_host_serving_consistent():
    """Device and host serving are the same process statistically: with the
    same seed and workload, job counts and energies land within a loose
    population band (different RNG streams for action sampling)."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess

    def run(mode):
        torch.manual_seed(5)
        sc = paper_scenario()
        inf = ArrivalProcess(mode="poisson", rate=2.0)
        trn = ArrivalProcess(mode="poisson", rate=0.2)
        eng = BatchedEngine(sc, inf, trn, algo="chsac_af", replicas=48,
                            duration=120.0, log_interval=5.0, out_dir=None,
                            seed=9, enable_logs=False, rl_warmup=10**9,
                            rl_serve=mode, events_per_launch=20000)
        st = eng.run()
        return (st["jobs_completed"] / 48.0,
                float(eng.t["energy_j"].sum().item()) / 48.0)

    jobs_d, en_d = run("device")
    jobs_h, en_h = run("host")
    assert abs(jobs_d - jobs_h) / max(jobs_h, 1) < 0.05
    assert abs(en_d - en_h) / en_h < 0.05


@needs_gpu
@pytest.mark.parametrize("inf_rate,trn_rate,elastic,duration", [
    (2.5, 0.3, False, 150.0),
    # saturating variant: heavy arrivals partially fill the pinned DC, so
    # admissions and drains get CLAMPED below the pinned n=8 — the regime
    # where reward-n bookkeeping (unclamped at arrival, clamped at drain)
    # can silently diverge
    (8.0, 0.3, False, 120.0),
    # elastic variant: training-only load long enough for completions, so
    # preempt-all + deterministic reallocation chains run on BOTH engines
    (0.0, 0.5, True, 1200.0),
])
def test_chsac_pinned_policy_parity(tmp_path, inf_rate, trn_rate, elastic,
                                    duration):
    """with a FROZEN agent served greedily (deterministic),
    the exact-p99 window enabled, and the oracle's recorded arrival trace,
    one GPU replica reproduces the oracle's chsac trajectory event-for-event
    — job log identical, and the recorded transitions (rewards, p99/gpu_over
    costs, masks) match, which pins the engine's RL mechanics including the
    exact percentile path (the fast path's histogram p99 stays the
    documented approximation)."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.engine.oracle import OracleEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,
                                                       CHSACAgentConfig)
    torch.manual_seed(42)
    agent = CHSACAgent(CHSACAgentConfig(
        obs_dim=49, n_dc=8, n_g_choices=8,
        constraints={"latency_p99": 500.0, "gpu_over": 0.0}, device="cuda"))
    # pin the greedy policy to (dc=2 — the 256-GPU DC, g=7 -> n=8): a frozen
    # random actor can wedge every job into a 16-GPU DC and starve the run;
    # this keeps churn high AND exercises free-GPU clamping on drains
    with torch.no_grad():
        for head, idx in ((agent.actor.head_dc[2], 2),
                          (agent.actor.head_g[2], 7)):
            head.weight.zero_()
            head.bias.zero_()
            head.bias[idx] = 10.0
    sc = paper_scenario()
    inf = ArrivalProcess(mode="poisson" if inf_rate > 0 else "off",
                         rate=inf_rate)
    trn = ArrivalProcess(mode="poisson", rate=trn_rate)
    rec = []
    out_o = str(tmp_path / "oracle")
    o_eng = OracleEngine(sc, inf, trn, algo="chsac_af", duration=duration,
                         log_interval=5.0, out_dir=out_o, seed=123,
                         rl_agent=agent, rl_warmup=10**9, rl_device="cuda",
                         rl_deterministic=True, arrival_recorder=rec,
                         elastic_scaling=elastic)
    # capture the oracle's reward-n per transition for divergence triage
    o_paths = []
    _orig_fin = o_eng._rl_on_finish

    def _fin(dc, job, g, f_used, rl_metrics):
        o_paths.append((int(job.jid), int(job.rl_action["n"]), int(g),
                        float(o_eng.now)))
        return _orig_fin(dc, job, g, f_used, rl_metrics)
    o_eng._rl_on_finish = _fin
    o_eng.run()

    ing_idx = {n: i for i, n in enumerate(sc.ingress_names)}
    NS = sc.n_ing * 2
    streams = [[] for _ in range(NS)]
    for (tt, ing, jtype, size, dc) in rec:
        s_id = ing_idx[ing] * 2 + (0 if jtype == "inference" else 1)
        streams[s_id].append((tt, size))
    cap = max(len(x) for x in streams) + 1
    times = np.full((1, NS, cap), 1e300)
    sizes = np.zeros((1, NS, cap), np.float64)
    for s_id, entries in enumerate(streams):
        for k, (tt, size) in enumerate(entries):
            times[0, s_id, k] = tt
            sizes[0, s_id, k] = size

    sc2 = paper_scenario()
    out_g = str(tmp_path / "gpu")
    eng = BatchedEngine(sc2, inf, trn, algo="chsac_af", replicas=1,
                        duration=duration, log_interval=5.0, out_dir=out_g,
                        seed=999, enable_logs=True, rl_agent=agent,
                        rl_warmup=10**9, rl_serve="host",
                        rl_deterministic=True, rl_exact_p99=True,
                        elastic_scaling=elastic,
                        arrival_trace=(times, sizes))
    eng.run()

    import pandas as pd
    jo = pd.read_csv(os.path.join(out_o, "job_log.csv"))
    jg = pd.read_csv(os.path.join(out_g, "job_log.csv"))
    assert len(jo) == len(jg), f"job count {len(jo)} vs {len(jg)}"
    jo = jo.sort_values("jid").reset_index(drop=True)
    jg = jg.sort_values("jid").reset_index(drop=True)
    for col in ("jid", "ingress", "type", "dc", "n_gpus"):
        assert (jo[col] == jg[col]).all(), f"column {col} diverged"
    for col, tol in (("size", 1e-9), ("f_used", 1e-12),
                     ("start_s", 1e-9), ("finish_s", 1e-9),
                     ("latency_s", 1e-9), ("preempt_count", 0)):
        d = (jo[col] - jg[col]).abs().max()
        assert d <= tol, f"column {col} max diff {d}"

    # transition-stream parity: same count, same actions/rewards/costs/masks
    # (costs carry the EXACT sliding-window p99 -> this pins the exact-p99
    # device path against the reference's np.percentile)
    if elastic:
        assert (jo["preempt_count"] > 0).any(), \
            "elastic parity is vacuous: no preemption occurred"
    orep, grep_ = o_eng.replay, eng.replay
    n = min(orep.size, grep_.size)
    # triage dump: full transition streams + oracle path info (merged back
    # through gpurun_out for offline analysis if an assert below trips)
    dbg_dir = os.path.join(REPO, "gpurun_out")
    if os.path.isdir(dbg_dir):
        np.savez(os.path.join(dbg_dir,
                              f"parity_dbg_el{int(elastic)}_r{inf_rate}.npz"),
                 r_o=orep.r[:n].cpu().numpy(), r_g=grep_.r[:n].cpu().numpy(),
                 s0_o=orep.s[:n].cpu().numpy(), s0_g=grep_.s[:n].cpu().numpy(),
                 sn_o=orep.s_next[:n].cpu().numpy(),
                 sn_g=grep_.s_next[:n].cpu().numpy(),
                 co=orep.costs[:n].cpu().numpy(),
                 cg=grep_.costs[:n].cpu().numpy(),
                 adc=orep.a_dc[:n].cpu().numpy(), ag=orep.a_g[:n].cpu().numpy(),
                 opaths=np.asarray(o_paths, np.float64))
    assert orep.size == grep_.size > (20 if elastic else 100), \
        (orep.size, grep_.size)
    assert torch.equal(orep.a_dc[:n].cpu(), grep_.a_dc[:n].cpu())
    assert torch.equal(orep.a_g[:n].cpu(), grep_.a_g[:n].cpu())
    assert torch.allclose(orep.r[:n].cpu(), grep_.r[:n].cpu(),
                          atol=1e-6, rtol=1e-5)
    oc = {name: orep.costs[:n, k].cpu()
          for k, name in enumerate(orep.cost_names)}
    gc = {name: grep_.costs[:n, k].cpu()
          for k, name in enumerate(grep_.cost_names)}
    assert torch.allclose(oc["latency_p99"], gc["latency_p99"],
                          atol=1e-4, rtol=1e-5), "exact-p99 cost diverged"
    assert torch.equal(oc["gpu_over"], gc["gpu_over"])
    assert torch.equal(orep.mask_dc[:n].cpu(), grep_.mask_dc[:n].cpu())
    assert torch.equal(orep.mask_g[:n].cpu(), grep_.mask_g[:n].cpu()), \
        "g-mask diverged (p99-vs-SLA cap path)"
    assert torch.allclose(orep.s[:n].cpu(), grep_.s[:n].cpu(), atol=1e-4)


@needs_gpu
def test_mfma_actor_forward_matches_torch():
    """The MFMA (matrix-core) batched actor forward must match the torch
    actor's logits within fp32 accumulation tolerance — fp32 MFMA is exact
    f32, so only summation order differs."""
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,
                                                       CHSACAgentConfig)
    mod = load_sim_hip()
    torch.manual_seed(17)
    obs_dim, n_dc, n_g, H = 49, 8, 8, 256
    agent = CHSACAgent(CHSACAgentConfig(
        obs_dim=obs_dim, n_dc=n_dc, n_g_choices=n_g,
        constraints={"latency_p99": 500.0}, device="cuda"))
    segs = []
    enc = agent.encoder.net
    for lin in (enc[0], enc[2], enc[4], agent.actor.head_dc[0],
                agent.actor.head_dc[2], agent.actor.head_g[0],
                agent.actor.head_g[2]):
        segs.append(lin.weight.detach().t().contiguous().reshape(-1))
        segs.append(lin.bias.detach().reshape(-1))
    pw = torch.cat(segs).float().cuda()
    for B in (1, 16, 250, 1024):   # incl. non-multiple-of-16 batch
        obs = torch.randn(B, obs_dim, device="cuda") * 50.0
        out_dc, out_g = mod.rl_forward_mfma(pw, obs, H, n_dc, n_g)
        with torch.no_grad():
            ref_dc, ref_g = agent.actor(agent.encoder(obs))
        for got, ref in ((out_dc, ref_dc), (out_g, ref_g)):
            diff = (got - ref).abs().max().item()
            scale = ref.abs().max().item() + 1.0
            assert diff <= 2e-4 * scale, f"B={B}: mfma diff {diff}"
    # and it agrees with the in-kernel serving forward (same buffer)
    obs = torch.randn(64, obs_dim, device="cuda")
    m_dc, m_g2 = mod.rl_forward_mfma(pw, obs, H, n_dc, n_g)
    d_dc, d_g = mod.rl_forward_debug(pw, obs, H, n_dc, n_g)
    assert (m_dc - d_dc).abs().max().item() < 1e-3
    assert (m_g2 - d_g).abs().max().item() < 1e-3


@needs_gpu
def test_chsac_host_serving_uses_mfma_forward():
    """Non-deterministic host serving routes the policy forward through the
    matrix-core kernel (production MFMA path), and the run behaves."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    inf = ArrivalProcess(mode="poisson", rate=1.5)
    trn = ArrivalProcess(mode="poisson", rate=0.2)
    eng = BatchedEngine(sc, inf, trn, algo="chsac_af", replicas=24,
                        duration=90.0, log_interval=5.0, out_dir=None,
                        seed=13, enable_logs=False, rl_serve="host",
                        rl_warmup=128, rl_batch=64, rl_train_interval=64,
                        events_per_launch=5000)
    assert eng._mfma_serve, "MFMA serving not enabled on the host path"
    st = eng.run()
    assert st["jobs_completed"] > 0
    assert eng.rl_updates > 0
    assert int(eng.t["err"].max().item()) == 0


@needs_gpu
def test_short_tensor_is_rejected_before_any_launch():
    """The extension's constructor checks every tensor's extent against what
    the kernel indexes: a state tensor one element short is a ValueError that
    names the field, raised before anything is launched."""
    from distributed_cluster_gpus_amd.engine.state import engine_cfg
    eng = make_engine(replicas=4, duration=20.0)
    cfg = engine_cfg(eng.dims, eng.sc, eng.arrival_inf, eng.arrival_trn)
    eng._mod.BatchedSimHip(eng.t, cfg)          # the engine's own state binds
    for field in ("q_pay", "s_rec", "busy"):
        bad = dict(eng.t)
        bad[field] = eng.t[field].reshape(-1)[:-1].clone()
        assert bad[field].is_cuda
        with pytest.raises(ValueError, match=f"'{field}': required"):
            eng._mod.BatchedSimHip(bad, cfg)
    assert int(eng.t["ev_count"].sum().item()) == 0   # nothing ran
