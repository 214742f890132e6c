"""Population time series on the MI355X: the reduce_series kernel on synthetic
data, and the advance kernel's per-replica sampling hook against the cluster
log, across builds, shards, strides, unfinished runs, checkpoints and the CLI.

Paper scenario, log_interval=5 (unless a test says otherwise), seed=123.
Tolerances are those of tests/test_pop_series_cpu.py: n / min / max exact,
mean rtol 1e-12, M2 rtol 1e-9 + atol 1e-9 * n * max|x - mean|^2."""
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

# cl_rows columns of the sampled metrics, in sample order
CL_COLS = [2, 3, 5, 8, 9, 13, 14]
K = len(CL_COLS)


def make_engine(algo="default_policy", replicas=16, duration=60.0,
                log_interval=5.0, enable_logs=False, **kw):
    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    sc = paper_scenario()
    inf, trn = build_arrivals()
    return BatchedEngine(sc, inf, trn, algo=algo, replicas=replicas,
                         duration=duration, log_interval=log_interval,
                         out_dir=None, seed=123, enable_logs=enable_logs, **kw)


def raw(eng):
    """(samples, ticks, time) on the host."""
    ps = eng.pop_samples()
    return ps["samples"].cpu(), ps["ticks"].cpu(), ps["time"].cpu()


def masked_reference(samples, ticks, every):
    """torch f64 masked two-pass reductions on the CPU: samples [T, C, R] ->
    (n, mean, m2, min, max, dev2) each [T, C]; dev2 = max|x - mean|^2."""
    T = samples.shape[0]
    mask = (ticks.to(torch.int64) // every).unsqueeze(0) > \
        torch.arange(T).unsqueeze(1)                        # [T, R]
    m = mask.unsqueeze(1)                                   # [T, 1, R]
    n = m.sum(dim=2).to(torch.float64).expand(T, samples.shape[1])
    nan = torch.full_like(n, float("nan"))
    # shift by the first contributing replica's sample, so that the
    # reference's own rounding is relative to the spread (and a cell of equal
    # samples has exactly that mean and M2 == 0)
    r0 = mask.to(torch.int64).argmax(dim=1)                 # [T]
    x0 = samples[torch.arange(T), :, r0].unsqueeze(2)       # [T, C, 1]
    mean = x0.squeeze(2) + torch.where(m, samples - x0, 0.0).sum(dim=2) / n
    dx = torch.where(m, samples - mean.unsqueeze(2), 0.0)
    m2 = (dx * dx).sum(dim=2)
    lo = torch.where(m, samples, float("inf")).amin(dim=2)
    hi = torch.where(m, samples, float("-inf")).amax(dim=2)
    some = n > 0
    return (n, torch.where(some, mean, nan), m2, torch.where(some, lo, nan),
            torch.where(some, hi, nan), (dx * dx).amax(dim=2))


def check_stats(got, ref):
    """got: [T, C, 5] from the kernel / SeriesStats; ref: masked_reference."""
    n, mean, m2, lo, hi, dev2 = ref
    assert torch.equal(got[..., 0], n)
    assert torch.equal(got[..., 3].nan_to_num(nan=-7.0), lo.nan_to_num(nan=-7.0))
    assert torch.equal(got[..., 4].nan_to_num(nan=-7.0), hi.nan_to_num(nan=-7.0))
    assert torch.equal(got[..., 1].isnan(), n == 0)
    some = n > 0
    assert torch.allclose(got[..., 1][some], mean[some], rtol=1e-12, atol=0.0)
    err = (got[..., 2] - m2).abs()
    bound = 1e-9 * m2.abs() + 1e-9 * n * dev2
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool((got[..., 2][~some] == 0).all())


def stats_tensor(st):
    """SeriesStats -> [T, C, 5] torch tensor."""
    a = torch.from_numpy(st.to_array())
    return a.reshape(a.shape[0], -1, 5)


# ---------------------------------------------------------------- kernel
@needs_gpu
@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_reduce_series_kernel_synthetic(R, every):
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    mod = load_sim_hip()
    g = torch.Generator().manual_seed(1000 * every + R)
    T, C = 3, 5
    x = torch.randn(T, C, R, generator=g, dtype=torch.float64) * \
        torch.tensor([1.0, 3.0, 50.0, 0.1, 1e3],
                     dtype=torch.float64).view(1, C, 1)
    # offsets keep every mean away from zero (a mean that cancels to ~0 has
    # no relative accuracy to speak of); column 0 is energy-like: 1e9 + N(0,1)
    x += torch.tensor([1e9, 10.0, -200.0, 0.5, 5e3],
                      dtype=torch.float64).view(1, C, 1)
    ticks = torch.randint(0, 4, (R,), generator=g, dtype=torch.int32)
    out = mod.reduce_series(x.cuda(), ticks.cuda(), every)
    again = mod.reduce_series(x.cuda(), ticks.cuda(), every)
    assert out.shape == (T, C, 5) and out.dtype == torch.float64
    assert torch.equal(out.cpu().nan_to_num(nan=-7.0),
                       again.cpu().nan_to_num(nan=-7.0))
    check_stats(out.cpu(), masked_reference(x, ticks, every))


# ---------------------------------------------------------------- sampling
@needs_gpu
@pytest.mark.parametrize("algo,kw", [
    ("default_policy", {}),
    ("cap_greedy", {"power_cap": 60000.0}),   # freq actually moves
])
def test_samples_equal_cluster_log(algo, kw):
    eng = make_engine(algo=algo, replicas=3, enable_logs=True,
                      pop_series=True, **kw)
    eng.run()
    n_dc = eng.sc.n_dc
    n_cl = int(eng.t["cl_count"].item())
    T = n_cl // n_dc
    assert T == 12 and n_cl == T * n_dc
    rows = eng.t["cl_rows"][:n_cl].cpu().view(T, n_dc, 15)
    samples, ticks, time = raw(eng)
    assert samples.shape == (12 // 1 + 2, n_dc + 1, K, 3)
    assert torch.equal(ticks, torch.full((3,), T, dtype=torch.int32))
    assert torch.equal(samples[:T, :n_dc, :, 0], rows[:, :, CL_COLS])
    assert torch.equal(time[:T], rows[:, 0, 0])
    assert bool((samples[T:] == 0).all())
    # fleet row, every replica: sum over the DC rows, mean for freq
    want = samples[:T, :n_dc].sum(dim=1)
    want[:, 0] = samples[:T, :n_dc, 0].mean(dim=1)
    assert torch.allclose(samples[:T, n_dc], want, rtol=1e-15 * n_dc, atol=0.0)
    if algo == "cap_greedy":
        f = samples[:T, :n_dc, 0]
        assert float(f.min()) < float(f.max()), "cap never moved a frequency"
    assert int(eng.t["err"].max().item()) == 0


@needs_gpu
def test_single_replica_series_is_the_logged_row():
    eng = make_engine(replicas=1, enable_logs=True, pop_series=True)
    eng.run()
    n_dc = eng.sc.n_dc
    n_cl = int(eng.t["cl_count"].item())
    T = n_cl // n_dc
    rows = eng.t["cl_rows"][:n_cl].cpu().view(T, n_dc, 15)
    st = eng.population_series()
    assert st.metrics == ["freq", "busy", "running", "q_inf", "q_trn",
                          "power_w", "energy_j"]
    assert st.dc_names == list(eng.sc.dc_names) + ["ALL"]
    assert st.n.shape == (T, n_dc + 1, K) and (st.n == 1).all()
    assert np.array_equal(st.time, rows[:, 0, 0].numpy())
    logged = rows[:, :, CL_COLS].numpy()
    for f in (st.mean, st.min, st.max):
        assert np.array_equal(f[:, :n_dc], logged)
    assert np.array_equal(st.mean[:, n_dc], st.min[:, n_dc])
    assert np.array_equal(st.mean[:, n_dc], st.max[:, n_dc])
    assert (st.m2 == 0).all()


@needs_gpu
def test_feature_off_and_on_same_trajectories():
    sys.path.insert(0, REPO)
    import bench
    on = make_engine(replicas=65, pop_series=True)
    on.run()
    off = make_engine(replicas=65)
    off.run()
    assert "ps_samples" not in off.t
    for name in bench.DUMP_TENSORS:
        assert torch.equal(on.t[name].cpu(), off.t[name].cpu()), name
    with pytest.raises(RuntimeError):
        off.pop_samples()


@pytest.fixture(scope="module")
def run16():
    """The replicas=16, every=1 run shared by the build and stride tests."""
    eng = make_engine(replicas=16, pop_series=True)
    eng.run()
    return raw(eng), stats_tensor(eng.population_series())


@needs_gpu
def test_subwave_builds_agree(run16):
    (s64, k64, t64), st64 = run16
    e8 = make_engine(replicas=16, pop_series=True, subwave=8)
    e8.run()
    s8, k8, t8 = raw(e8)
    assert torch.equal(s64, s8) and torch.equal(k64, k8)
    assert torch.equal(t64, t8)
    assert torch.equal(st64, stats_tensor(e8.population_series()))


@needs_gpu
def test_stride_takes_every_third_tick(run16):
    (s1, k1, t1), _ = run16
    e3 = make_engine(replicas=16, pop_series=True, pop_series_every=3)
    e3.run()
    s3, k3, t3 = raw(e3)
    assert s3.shape[0] == 12 // 3 + 2
    assert torch.equal(k3, k1) and int(k1[0]) == 12   # ticks count log ticks
    assert torch.equal(s3[:4], s1[2:12:3])            # ticks 3, 6, 9, 12
    assert torch.equal(t3[:4], t1[2:12:3])
    assert bool((s3[4:] == 0).all())
    st = e3.population_series()
    assert np.array_equal(st.time, t1[2:12:3].numpy())
    assert (st.n == 16).all()


@needs_gpu
def test_shards_reproduce_the_full_run():
    from distributed_cluster_gpus_amd.analysis.montecarlo import \
        merge_series_stats
    full = make_engine(replicas=8, pop_series=True)
    full.run()
    lo = make_engine(replicas=8, pop_series=True, rank=0, world=2)
    lo.run()
    hi = make_engine(replicas=8, pop_series=True, rank=1, world=2)
    hi.run()
    sf, kf, tf = raw(full)
    sl, kl, tl = raw(lo)
    sh, kh, th = raw(hi)
    assert torch.equal(sf[..., :4], sl) and torch.equal(sf[..., 4:], sh)
    assert torch.equal(kf[:4], kl) and torch.equal(kf[4:], kh)
    assert torch.equal(tf, tl) and torch.equal(tf, th)
    merged = merge_series_stats([lo.population_series(),
                                 hi.population_series()])
    T = int(kf[0])
    ref = masked_reference(sf[:T].reshape(T, -1, 8), kf, 1)
    check_stats(stats_tensor(merged), ref)
    check_stats(stats_tensor(full.population_series()), ref)
    assert np.array_equal(merged.time, tf[:T].numpy())


@needs_gpu
def test_unfinished_run_counts_per_tick():
    """One event-bounded launch leaves the replicas at different times.  The
    budget has to end them AROUND a tick boundary for the tick counters to
    differ: the paper workload runs ~230 events per simulated second per
    replica (profiles/README.md, whole-workload table: 141.5 M events / 512
    replicas / 1200 s; the sinusoid starts at its mean rate), and after a few
    hundred events the replicas are spread over a few tenths of a second.  A
    budget of 300 ends every replica inside (1 s, 2 s) — all counters equal,
    nothing to test — so the budget is 460: t ~ 2.0 s, some replicas before
    the second tick and some past it."""
    eng = make_engine(replicas=64, log_interval=1.0, pop_series=True)
    eng._sim.advance(eng.end_time, 460)
    torch.cuda.synchronize()
    samples, ticks, time = raw(eng)
    assert int(ticks.min()) < int(ticks.max()), "replicas did not drift apart"
    st = eng.population_series()
    T = int(ticks.max())
    assert st.n.shape[0] == T
    for t in range(T):
        assert (st.n[t] == int((ticks > t).sum())).all(), t
    check_stats(stats_tensor(st),
                masked_reference(samples[:T].reshape(T, -1, 64), ticks, 1))
    assert np.array_equal(st.time, time[:T].numpy())


@needs_gpu
def test_checkpoint_continues_the_series(tmp_path):
    eng = make_engine(replicas=16, pop_series=True)
    eng._sim.advance(30.0, 10**9)
    torch.cuda.synchronize()
    ckpt = str(tmp_path / "state.pt")
    eng.save_state(ckpt)
    mid = raw(eng)
    assert 0 < int(mid[1].max()) < 12
    eng.run()
    a = raw(eng)
    eng2 = make_engine(replicas=16, pop_series=True)
    eng2.load_state(ckpt)
    assert torch.equal(raw(eng2)[1], mid[1])
    eng2.run()
    b = raw(eng2)
    assert int(a[1].min()) == 12
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@needs_gpu
def test_cli_writes_population_series(tmp_path):
    import pandas as pd
    out = str(tmp_path / "cli" / "run")
    r = subprocess.run([sys.executable, os.path.join(REPO, "run_sim.py"),
                        "--engine", "batched", "--replicas", "16",
                        "--duration", "60", "--pop-series",
                        "--log-path", out, "--progress", "False"],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    df = pd.read_csv(os.path.join(out, "population", "population_series.csv"),
                     keep_default_na=False, na_values=[""])
    assert list(df.columns) == ["time_s", "dc", "metric", "n", "mean", "std",
                                "stderr", "ci_lo", "ci_hi", "min", "max"]
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    n_dc = paper_scenario().n_dc
    per_tick = df.groupby("time_s").size()
    assert len(per_tick) == 12 and (per_tick == (n_dc + 1) * K).all()
    assert (df["n"] == 16).all()
    assert set(df["dc"]) >= {"ALL"} and len(set(df["dc"])) == n_dc + 1
    assert os.path.exists(os.path.join(out, "population", "population.csv"))
    assert os.path.exists(os.path.join(
        out, "population", "population_series_fleet_power.csv"))
    with open(os.path.join(out, "project.log")) as fh:
        assert "pop_series: sample buffer" in fh.read()
