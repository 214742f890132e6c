"""Analysis-layer tests: run loading, aggregation, all figure artifacts."""
import os

import numpy as np
import pandas as pd
import pytest

from distributed_cluster_gpus_amd.analysis.aggregate import (aggregate_cluster,
                                                             load_run,
                                                             summarize_run)
from distributed_cluster_gpus_amd.analysis.plots import (COMPARISON_FIGURES,
                                                         comparison_report)
from distributed_cluster_gpus_amd.analysis.plots_single import (SINGLE_FIGURES,
                                                                single_algo_report)
from distributed_cluster_gpus_amd.configs.paper import build_arrivals, paper_scenario
from distributed_cluster_gpus_amd.engine.native import NativeEngine


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("runs")
    dirs = {}
    for algo in ("default_policy", "joint_nf"):
        sc = paper_scenario()
        inf, trn = build_arrivals()
        out = str(base / algo)
        NativeEngine(sc, inf, trn, algo=algo, duration=60.0, log_interval=5.0,
                     out_dir=out, seed=123).run()
        dirs[algo] = out
    return dirs


def test_load_and_aggregate(two_runs):
    cluster, jobs = load_run(two_runs["default_policy"])
    assert set(cluster.columns) >= {"time_s", "dc", "power_W", "energy_kJ"}
    agg = aggregate_cluster(cluster)
    assert (agg["power_W"] > 0).all()
    # cumulative energy is monotonic
    assert agg["energy_kJ"].is_monotonic_increasing
    # 8 DCs per tick folded into one row per tick
    assert len(agg) == cluster["time_s"].nunique()


def test_summarize(two_runs):
    s = summarize_run(two_runs["default_policy"])
    assert s["jobs_completed"] > 0
    assert s["total_energy_kJ"] > 0
    assert s["mean_inf_latency_s"] > 0
    assert s["energy_per_unit_J"] > 0


def test_comparison_report_artifacts(two_runs, tmp_path):
    out = str(tmp_path / "report")
    arts = comparison_report(two_runs, out)
    produced = {os.path.splitext(os.path.basename(a))[0] for a in arts}
    for fig in COMPARISON_FIGURES:
        assert os.path.exists(os.path.join(out, f"{fig}.csv")), fig
    assert os.path.exists(os.path.join(out, "summary.csv"))
    summary = pd.read_csv(os.path.join(out, "summary.csv"))
    assert set(summary["algo"]) == {"default_policy", "joint_nf"}
    # the reference's headline claim shows up in the data: joint_nf uses less
    # energy than default_policy
    e = summary.set_index("algo")["total_energy_kJ"]
    assert e["joint_nf"] < e["default_policy"]


def test_single_report_artifacts(two_runs, tmp_path):
    from distributed_cluster_gpus_amd.configs.paper import (DC_GPUS_LABEL,
                                                            GW_ALPHABET_LABEL)
    out = str(tmp_path / "single")
    single_algo_report(two_runs["default_policy"], out,
                       dc_labels=DC_GPUS_LABEL, gw_labels=GW_ALPHABET_LABEL)
    for fig in SINGLE_FIGURES:
        assert os.path.exists(os.path.join(out, f"{fig}.csv")), fig
    heat = pd.read_csv(os.path.join(out, "routing_heatmap.csv"))
    assert len(heat) == 8  # 8 ingresses
    assert len(heat.columns) == 9  # ingress + 8 DCs


def test_plot_cli(two_runs, tmp_path):
    import plot_results
    import plot_single
    out = str(tmp_path / "cli_report")
    arts = plot_results.main(["--runs"] +
                             [f"{k}={v}" for k, v in two_runs.items()] +
                             ["--out", out])
    assert len(arts) >= 13
    out2 = str(tmp_path / "cli_single")
    arts2 = plot_single.main(["--run", two_runs["default_policy"],
                              "--out", out2])
    assert len(arts2) == len(SINGLE_FIGURES)


def test_plot_sh_wrapper(two_runs, tmp_path):
    """plot.sh discovers run subdirectories and emits the full report."""
    import shutil
    import subprocess
    import sys
    root = str(tmp_path / "runs_root")
    os.makedirs(root)
    for name, d in two_runs.items():
        shutil.copytree(d, os.path.join(root, name))
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["bash", os.path.join(repo, "plot.sh"), root],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert os.path.exists(os.path.join(root, "report", "summary.csv"))


def test_violin_and_boxen_render(tmp_path):
    """The violin / letter-value latency views render as PNGs (matplotlib is
    present here) and always emit their CSV data artifacts."""
    import numpy as np
    import pandas as pd
    from distributed_cluster_gpus_amd.analysis.render import emit, have_mpl
    rng = np.random.default_rng(0)
    df = pd.DataFrame({
        "latency_s": np.concatenate([rng.exponential(0.01, 400),
                                     rng.exponential(0.05, 400)]),
        "algo": ["a"] * 400 + ["b"] * 400,
    })
    for kind in ("violin", "boxen"):
        path = emit(df, str(tmp_path), f"lat_{kind}", kind=kind,
                    y="latency_s", hue="algo", title=kind)
        assert os.path.exists(os.path.join(str(tmp_path), f"lat_{kind}.csv"))
        if have_mpl():
            assert os.path.exists(os.path.join(str(tmp_path),
                                               f"lat_{kind}.png"))


# ---------------- the shared ensemble moments ----------------
MOMENT_FIELDS = ("n", "mean", "m2", "min", "max")


def _wrap_three(a):
    """The same [4, 3, 5] cell array as a SeriesStats (4 ticks x 3 DCs x 1
    metric), a LatencyStats (2 rows x 2 job types x 3 figures, empty
    histograms) and a SweepStats (4 groups x 3 metrics)."""
    from distributed_cluster_gpus_amd.analysis.montecarlo import (
        LH_BINS, LatencyStats, SeriesStats, SweepStats)
    return (
        SeriesStats.from_tensor(a.reshape(4, 3, 1, 5), np.arange(4.0),
                                metrics=["m"], dc_names=["a", "b", "ALL"]),
        LatencyStats.from_tensor(np.zeros((2, 2, LH_BINS), np.int64),
                                 a.reshape(2, 2, 3, 5), quantiles=[0.5],
                                 dc_names=["a", "ALL"], sla_s=1.0),
        SweepStats.from_array(a, metrics=["x", "y", "z"]))


def test_one_merge_behind_the_three_statistics():
    """merge_series_stats, merge_latency_stats and merge_sweep_stats over the
    same cells give the same bytes, those of Moments.merge folded in the same
    tree order; some cells are empty on one side, on both, or hold one
    replica."""
    from distributed_cluster_gpus_amd.analysis.montecarlo import (
        Moments, merge_latency_stats, merge_series_stats, merge_sweep_stats)
    rng = np.random.default_rng(11)
    x = rng.normal(size=(10, 4, 3)) * 3.0 + 1e6
    x[:, 0, 0] = np.nan           # no replica has the figure: n = 0 everywhere
    x[1:, 0, 1] = np.nan          # one replica has it: n = 1 in one part
    x[:5, 0, 2] = np.nan          # the first parts hold none of it
    x[::3, 2, 1] = np.nan

    def cells(rows):
        m = Moments.from_values(x[rows].reshape(len(rows), 12),
                                [(0, len(rows))])
        return m.to_array().reshape(4, 3, 5)

    for k in (1, 2, 3, 5):
        arrays = [cells(rows) for rows in np.array_split(np.arange(10), k)]
        n = np.stack([a[..., 0] for a in arrays])
        assert (n[:, 0, 0] == 0).all() and sorted(n[:, 0, 1])[-1] == 1
        if k > 1:
            assert n[0, 0, 2] == 0 and n[-1, 0, 2] > 0
        ref = [Moments.from_array(a) for a in arrays]
        while len(ref) > 1:
            nxt = [Moments.merge(ref[i], ref[i + 1])
                   for i in range(0, len(ref) - 1, 2)]
            ref = nxt + ref[len(ref) - len(ref) % 2:]
        wrapped = [_wrap_three(a) for a in arrays]
        merged = (merge_series_stats([w[0] for w in wrapped]),
                  merge_latency_stats([w[1] for w in wrapped]),
                  merge_sweep_stats([w[2] for w in wrapped]))
        for f in MOMENT_FIELDS:
            want = getattr(ref[0], f)
            assert want.dtype == (np.int64 if f == "n" else np.float64)
            for got in merged:
                assert getattr(got, f).dtype == want.dtype
                assert getattr(got, f).tobytes() == want.tobytes(), (k, f)
        # the whole ensemble, reduced in one piece
        whole = cells(np.arange(10))
        assert np.array_equal(merged[2].n, whole[..., 0])
        np.testing.assert_allclose(merged[2].mean, whole[..., 1], rtol=1e-12)


def test_one_spread_behind_the_three_frames():
    """std / stderr are 0 where n < 2 and never NaN, also where rounding left
    a tiny negative m2; the three frames print the same error bars."""
    from distributed_cluster_gpus_amd.analysis.montecarlo import (
        LH_BINS, LatencyStats, Moments, SeriesStats, SweepStats,
        latency_frame, series_frame, sweep_frame)
    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    n = np.array([0, 1, 2, 7, 0, 1, 2, 7], np.int64)
    m2 = np.array([0.0, 0.0, -1e-18, -1e-18, 0.0, -1e-18, 3.0, 12.5])
    mean = np.where(n > 0, 5.0 + np.arange(8), np.nan)
    a = np.stack([n.astype(np.float64), mean, m2, mean - 1, mean + 1],
                 axis=-1)
    m = Moments.from_array(a)
    std, se = m.std(), m.stderr()
    assert not np.isnan(std).any() and not np.isnan(se).any()
    assert (std[n < 2] == 0).all() and (se[n < 2] == 0).all()
    assert (std[:6] == 0).all() and (se[:6] == 0).all()   # clamped m2
    assert std[6] == np.sqrt(3.0 / 1) and se[6] == std[6] / np.sqrt(2)
    assert std[7] == np.sqrt(12.5 / 6) and se[7] == std[7] / np.sqrt(7)

    sf = series_frame(SeriesStats.from_tensor(
        a.reshape(8, 1, 1, 5), np.arange(8.0), metrics=["m"],
        dc_names=["ALL"]))
    lf = latency_frame(LatencyStats.from_tensor(
        np.zeros((2, 2, LH_BINS), np.int64), a.reshape(2, 2, 2, 5),
        quantiles=[], dc_names=["a", "ALL"], sla_s=1.0))
    wf = sweep_frame(SweepStats.from_array(a.reshape(8, 1, 5), metrics=["m"]),
                     Sweep.grid(inf_rate=list(range(1, 9))))
    z = 1.96
    want = {"std": std, "stderr": se, "ci_lo": mean - z * se,
            "ci_hi": mean + z * se}
    for col, w in want.items():
        assert sf[col].to_numpy().tobytes() == w.tobytes(), col
        assert lf[col].to_numpy().tobytes() == w.tobytes(), col
        if col != "std":          # sweep_frame has no std column
            assert wf[f"m_{col}"].to_numpy().tobytes() == w.tobytes(), col
