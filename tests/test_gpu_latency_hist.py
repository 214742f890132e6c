"""Per-replica latency histograms on the MI355X: the latency_reduce kernels on
synthetic data, and the advance kernel's job-finish hook against the job log,
across builds, shards, checkpoints, chsac_af and the CLI.

Paper scenario, 60 s, seed=123 (and the same run carried on to 600 s where a
test needs training jobs to finish: none does in the first 60 s).  Statistics
are held as
tests/test_gpu_pop_series.py holds them: n / min / max exact, mean rtol 1e-12,
M2 rtol 1e-9 + atol 1e-9 * n * max|x - mean|^2.  Integer results (histograms,
counts) and quantiles (bin edges) are held exactly."""
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

QS = (0.5, 0.9, 0.99, 0.999)
LO, LAST = 2.0 ** -14, 1.875 * 2.0 ** 17     # the exact range of the bound
B = 256


def make_engine(algo="default_policy", replicas=16, duration=60.0,
                enable_logs=False, **kw):
    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    sc = paper_scenario()
    inf, trn = build_arrivals()
    return BatchedEngine(sc, inf, trn, algo=algo, replicas=replicas,
                         duration=duration, log_interval=5.0, out_dir=None,
                         seed=123, enable_logs=enable_logs, **kw)


def raw(eng):
    lh = eng.latency_hist()
    return lh["hist"].cpu(), lh["over"].cpu()


def upper_edges():
    """Upper bin edges by ldexp: 8 bins per octave from 2^-14 s."""
    up = np.array([np.ldexp(1.0 + ((b + 1) % 8) / 8.0, (b + 1) // 8 - 14)
                   for b in range(B)])
    up[B - 1] = np.inf
    return up


def reference(hist, over, qs):
    """numpy: (pop_hist[C', B], per_rep[C', K, R]) from hist [R, D, 2, B] and
    over [R, D, 2]; row D = sum over DCs."""
    hist, over = hist.astype(np.int64), over.astype(np.int64)
    R, D = hist.shape[:2]
    h = np.concatenate([hist, hist.sum(axis=1, keepdims=True)], axis=1)
    o = np.concatenate([over, over.sum(axis=1, keepdims=True)], axis=1)
    pop = h.sum(axis=0).reshape((D + 1) * 2, B)
    K = len(qs) + 2
    per = np.full(((D + 1) * 2, K, R), np.nan)
    up = upper_edges()
    for r in range(R):
        for c in range((D + 1) * 2):
            cum = np.cumsum(h[r, c // 2, c % 2])
            n = int(cum[-1])
            per[c, K - 1, r] = n
            if n == 0:
                continue
            for k, q in enumerate(qs):
                rank = int(np.ceil(q * float(n)))
                per[c, k, r] = up[np.searchsorted(cum, rank, side="left")]
            per[c, K - 2, r] = o[r, c // 2, c % 2] / n
    return pop, per


def check_stats(got, per):
    """got [C', K, 5] against the rows of per [C', K, R] (NaN = no value)."""
    for c in range(per.shape[0]):
        for k in range(per.shape[1]):
            v = per[c, k][~np.isnan(per[c, k])]
            g = got[c, k]
            assert g[0] == len(v), (c, k)
            if len(v) == 0:
                assert np.isnan(g[1]) and g[2] == 0 and np.isnan(g[3]) \
                    and np.isnan(g[4]), (c, k)
                continue
            assert g[3] == v.min() and g[4] == v.max(), (c, k)
            if np.isinf(v).any():       # no finite mean to speak of
                assert g[1] == np.inf, (c, k)
                continue
            mean = v[0] + (v - v[0]).sum() / len(v)
            m2 = ((v - mean) ** 2).sum()
            dev2 = ((v - mean) ** 2).max()
            assert np.isclose(g[1], mean, rtol=1e-12, atol=0.0), (c, k)
            assert abs(g[2] - m2) <= 1e-9 * abs(m2) + 1e-9 * len(v) * dev2, \
                (c, k, g[2], m2)


def job_rows(eng):
    """The logging replica's job rows: (dc, type, sojourn) arrays."""
    n = int(eng.t["jl_count"].item())
    rows = np.concatenate(list(eng._jl_chunks) +
                          [eng.t["jl_rows"][:n].cpu().numpy()], axis=0)
    return rows[:, 4].astype(int), rows[:, 2].astype(int), \
        np.maximum(rows[:, 9] - rows[:, 8], 0.0)


# ---------------------------------------------------------------- kernels
@needs_gpu
@pytest.mark.parametrize("Q", [1, 4, 8])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 257])
def test_latency_reduce_synthetic(R, Q):
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    mod = load_sim_hip()
    rng = np.random.default_rng(1000 * Q + R)
    D = 3
    qs = [(0.5,), QS, (0.01, 0.25, 0.5, 0.75, 0.9, 0.99, 0.999, 1.0)][
        (1, 4, 8).index(Q)]
    hist = np.zeros((R, D, 2, B), np.int32)
    hist[..., 40:200] = rng.integers(0, 50, (R, D, 2, 160)) * \
        (rng.random((R, D, 2, 160)) < 0.3)
    hist[rng.random((R, D, 2)) < 0.2] = 0       # empty (replica, cell)s
    hist[:, 1, 1] = 0                           # a cell empty in every replica
    hist[:, 2, 0] = 0                           # a cell wholly in bin 255
    hist[:, 2, 0, 255] = rng.integers(1, 4, R)
    hist[0, 0, 0] = 0                           # everything in bin 0
    hist[0, 0, 0, 0] = 17
    hist[R - 1, 1, 0] = 0                       # a single sample
    hist[R - 1, 1, 0, 123] = 1
    count = hist.sum(axis=-1)
    over = (rng.random((R, D, 2)) * (count + 1)).astype(np.int32)
    over = np.minimum(over, count).astype(np.int32)
    args = (torch.from_numpy(hist).cuda(), torch.from_numpy(over).cuda(),
            torch.tensor(qs, dtype=torch.float64))
    pop, per, stats = (x.cpu().numpy() for x in mod.latency_reduce(*args))
    again = [x.cpu().numpy() for x in mod.latency_reduce(*args)]
    C, K = (D + 1) * 2, Q + 2
    assert pop.shape == (C, B) and pop.dtype == np.int64
    assert per.shape == (C, K, R) and stats.shape == (C, K, 5)
    for a, b in zip((pop, per, stats), again):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    ref_pop, ref_per = reference(hist, over, qs)
    assert np.array_equal(pop, ref_pop)
    assert np.array_equal(np.isnan(per), np.isnan(ref_per))
    assert np.array_equal(per, ref_per, equal_nan=True)
    # the planted cells say what they must
    assert (per[2 * 2 + 0, :Q] == np.inf).all()
    assert (per[0, :Q, 0] == 1.125 * LO).all()
    assert np.isnan(per[1 * 2 + 1, :Q + 1]).all() and \
        (per[1 * 2 + 1, Q + 1] == 0).all()
    assert (per[1 * 2 + 0, :Q, R - 1] == upper_edges()[123]).all()
    assert not np.isnan(per[:, K - 1]).any()
    check_stats(stats, ref_per)
    assert stats[1 * 2 + 1, 0, 0] == 0 and stats[0, K - 1, 0] == R


# ---------------------------------------------------------------- recording
@pytest.fixture(scope="module")
def logged3():
    """replicas=3 with the job log, default SLA: shared by the recording and
    the quantile-bound tests."""
    eng = make_engine(replicas=3, enable_logs=True, latency_hist=True)
    eng.run()
    return eng


def check_recording(eng, sla_s):
    hist, over = raw(eng)
    n_dc = eng.sc.n_dc
    assert hist.shape == (3, n_dc, 2, B) and hist.dtype == torch.int32
    assert over.shape == (3, n_dc, 2) and over.dtype == torch.int32
    from distributed_cluster_gpus_amd.analysis.montecarlo import \
        latency_histogram
    dc, jt, x = job_rows(eng)
    assert len(x) > 0
    for d in range(n_dc):
        for j in range(2):
            sel = x[(dc == d) & (jt == j)]
            assert np.array_equal(hist[0, d, j].numpy(),
                                  latency_histogram(sel)), (d, j)
            assert int(over[0, d, j]) == int((sel > sla_s).sum()), (d, j)
    per_type = hist.sum(dim=(1, 3)).to(torch.int64)          # [R, 2]
    done, inf = eng.t["jobs_done"].cpu(), eng.t["jobs_done_inf"].cpu()
    assert torch.equal(per_type[:, 0], inf)
    assert torch.equal(per_type[:, 1], done - inf)
    assert int(done.min()) > 0
    assert int(eng.t["err"].max().item()) == 0
    return int(over.sum()), int(hist.sum())


@needs_gpu
def test_recording_equals_job_log_default_policy(logged3):
    assert logged3.latency_hist()["sla_s"] == 0.5
    check_recording(logged3, 0.5)


@needs_gpu
@pytest.mark.parametrize("algo,kw", [
    ("default_policy", {"latency_sla_s": 0.05}),
    ("cap_greedy", {"power_cap": 60000.0}),
    ("cap_greedy", {"power_cap": 60000.0, "latency_sla_s": 0.05}),
])
def test_recording_equals_job_log(algo, kw):
    eng = make_engine(algo=algo, replicas=3, enable_logs=True,
                      latency_hist=True, **kw)
    eng.run()
    sla_s = kw.get("latency_sla_s", 0.5)
    n_over, n_all = check_recording(eng, sla_s)
    if "latency_sla_s" in kw:
        assert 0 < n_over < n_all, "the SLA separates nothing"


@pytest.fixture(scope="module")
def logged3_long():
    """The same run carried on to 600 s (same seed: its first 60 s are the
    run above).  On the paper scenario the first training job finishes after
    about 290 s, so a 60 s run has no training sojourn at all."""
    eng = make_engine(replicas=3, duration=600.0, enable_logs=True,
                      latency_hist=True)
    eng.run()
    return eng


@needs_gpu
def test_recording_equals_job_log_with_training(logged3_long):
    check_recording(logged3_long, 0.5)
    done = logged3_long.t["jobs_done"].cpu()
    assert int((done - logged3_long.t["jobs_done_inf"].cpu()).min()) > 0


@needs_gpu
@pytest.mark.parametrize("which", ["60s", "600s"])
def test_quantile_bound_on_real_data(which, logged3, logged3_long):
    """Replica 0, every DC row and the fleet row.  The 60 s run holds the
    bound for inference only (no training job finishes that early); the
    600 s run must have both job types in range."""
    eng = logged3 if which == "60s" else logged3_long
    hist, over = raw(eng)
    n_dc = eng.sc.n_dc
    _, per, _ = eng._mod.latency_reduce(
        hist.cuda(), over.cuda(), torch.tensor(QS, dtype=torch.float64))
    per = per.cpu().numpy()
    dc, jt, x = job_rows(eng)
    in_range = [0, 0]
    for row in range(n_dc + 1):
        for j in range(2):
            sel = np.sort(x[((dc == row) | (row == n_dc)) & (jt == j)])
            if len(sel) == 0:
                assert np.isnan(per[row * 2 + j, :len(QS), 0]).all()
                continue
            for k, q in enumerate(QS):
                true = sel[int(np.ceil(q * float(len(sel)))) - 1]
                v = per[row * 2 + j, k, 0]
                if LO <= true < LAST:
                    assert true < v <= 1.125 * true, (row, j, q, true, v)
                    in_range[j] += 1
            assert per[row * 2 + j, len(QS) + 1, 0] == len(sel)
    assert in_range[0] > 0, in_range
    if which == "600s":
        assert in_range[1] > 0, in_range
    else:
        assert not (jt == 1).any(), "a training job finished within 60 s"


@needs_gpu
def test_feature_off_and_on_same_trajectories():
    sys.path.insert(0, REPO)
    import bench
    on = make_engine(replicas=65, latency_hist=True)
    on.run()
    off = make_engine(replicas=65)
    off.run()
    assert "lh_hist" not in off.t and "lh_over" not in off.t
    assert int(on.t["lh_hist"].sum()) == int(on.t["jobs_done"].sum())
    for name in bench.DUMP_TENSORS:
        assert torch.equal(on.t[name].cpu(), off.t[name].cpu()), name
    with pytest.raises(RuntimeError):
        off.latency_hist()
    with pytest.raises(RuntimeError):
        off.latency_distribution()


@needs_gpu
def test_subwave_builds_agree():
    e64 = make_engine(replicas=16, latency_hist=True)
    e64.run()
    e8 = make_engine(replicas=16, latency_hist=True, subwave=8)
    e8.run()
    for a, b in zip(raw(e64), raw(e8)):
        assert torch.equal(a, b)
    assert int(raw(e64)[0].sum()) > 0


@needs_gpu
def test_shards_reproduce_the_full_run():
    from distributed_cluster_gpus_amd.analysis.montecarlo import \
        merge_latency_stats
    full = make_engine(replicas=8, latency_hist=True)
    full.run()
    lo = make_engine(replicas=8, latency_hist=True, rank=0, world=2)
    lo.run()
    hi = make_engine(replicas=8, latency_hist=True, rank=1, world=2)
    hi.run()
    (hf, of), (hl, ol), (hh, oh) = raw(full), raw(lo), raw(hi)
    assert torch.equal(hf[:4], hl) and torch.equal(hf[4:], hh)
    assert torch.equal(of[:4], ol) and torch.equal(of[4:], oh)
    merged = merge_latency_stats([lo.latency_distribution(),
                                  hi.latency_distribution()])
    whole = full.latency_distribution()
    n_row = full.sc.n_dc + 1
    assert whole.dc_names == list(full.sc.dc_names) + ["ALL"]
    assert whole.metrics == ["p50", "p90", "p99", "p99.9", "sla_miss_frac",
                             "jobs"]
    assert whole.pop_hist.shape == (n_row, 2, B)
    assert np.array_equal(whole.pop_hist[-1].sum(axis=-1),
                          hf.sum(dim=(0, 1, 3)).numpy())
    ref_pop, ref_per = reference(hf.numpy(), of.numpy(), QS)
    for st in (merged, whole):
        assert np.array_equal(st.pop_hist.reshape(-1, B), ref_pop)
        check_stats(st.to_array().reshape(n_row * 2, len(QS) + 2, 5), ref_per)
    assert np.array_equal(merged.n, whole.n)
    assert np.array_equal(merged.min, whole.min, equal_nan=True)
    assert np.array_equal(merged.max, whole.max, equal_nan=True)
    assert (whole.n[-1, :, -1] == 8).all()       # every replica has a count


@needs_gpu
def test_checkpoint_continues_the_histograms(tmp_path):
    eng = make_engine(replicas=16, latency_hist=True)
    eng._sim.advance(30.0, 10**9)
    torch.cuda.synchronize()
    ckpt = str(tmp_path / "state.pt")
    eng.save_state(ckpt)
    mid = raw(eng)
    eng.run()
    a = raw(eng)
    assert 0 < int(mid[0].sum()) < int(a[0].sum())
    eng2 = make_engine(replicas=16, latency_hist=True)
    eng2.load_state(ckpt)
    assert torch.equal(raw(eng2)[0], mid[0])
    eng2.run()
    b = raw(eng2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # a checkpoint of a run without the histograms does not load into one with
    off = make_engine(replicas=16)
    with pytest.raises(ValueError):
        off.load_state(ckpt)


@needs_gpu
def test_chsac_counts_every_finish():
    eng = make_engine(algo="chsac_af", replicas=8, duration=30.0,
                      latency_hist=True, rl_warmup=10**9,
                      events_per_launch=5000)
    eng.run()
    hist, _ = raw(eng)
    per_type = hist.sum(dim=(1, 3)).to(torch.int64)
    assert torch.equal(per_type, eng.t["lat_count"].cpu())
    assert int(per_type.sum()) > 0
    assert int(eng.t["err"].max().item()) == 0


@needs_gpu
def test_cli_writes_latency_reports(tmp_path):
    import pandas as pd
    out = str(tmp_path / "cli" / "run")
    r = subprocess.run([sys.executable, os.path.join(REPO, "run_sim.py"),
                        "--engine", "batched", "--replicas", "16",
                        "--duration", "60", "--latency-hist",
                        "--log-path", out, "--progress", "False"],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    df = pd.read_csv(os.path.join(out, "population", "latency_quantiles.csv"),
                     keep_default_na=False, na_values=[""])
    assert list(df.columns) == ["dc", "type", "metric", "n", "mean", "std",
                                "stderr", "ci_lo", "ci_hi", "min", "max"]
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    n_dc = paper_scenario().n_dc
    assert len(df) == (n_dc + 1) * 2 * 6
    assert set(df["dc"]) >= {"ALL"} and len(set(df["dc"])) == n_dc + 1
    assert set(df["type"]) == {"inference", "training"}
    jobs = df[df["metric"] == "jobs"]
    assert len(jobs) == (n_dc + 1) * 2 and (jobs["n"] == 16).all()
    fleet = df[(df["dc"] == "ALL") & (df["type"] == "inference")]
    assert (fleet["n"] == 16).all() and fleet["mean"].notna().all()
    hf = pd.read_csv(os.path.join(out, "population", "latency_hist.csv"))
    assert list(hf.columns) == ["dc", "type", "bin_lo_s", "bin_hi_s", "count"]
    assert (hf["count"] > 0).all() and (hf["bin_lo_s"] < hf["bin_hi_s"]).all()
    fleet_jobs = hf[hf["dc"] == "ALL"]["count"].sum()
    assert fleet_jobs == hf[hf["dc"] != "ALL"]["count"].sum() > 0
    with open(os.path.join(out, "project.log")) as fh:
        log = fh.read()
    assert "latency_hist: 16 replicas" in log
    assert "latency_hist: inference pooled p99" in log
    assert "latency_hist: training pooled p99" in log
