"""Latency statistics on the host (analysis/montecarlo.py) and the latency
histograms' place in the engine state (engine/state.py), no GPU.

Tolerances for merged statistics are those of tests/test_gpu_pop_series.py:
n / min / max and histograms exact, mean rtol 1e-12, M2 rtol 1e-9 + atol
1e-9 * n * max|x - mean|^2."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from distributed_cluster_gpus_amd.analysis.montecarlo import (  # noqa: E402
    DEFAULT_QUANTILES, LatencyStats, latency_bin_edges, latency_bins,
    latency_frame, latency_hist_frame, latency_histogram, latency_quantile,
    merge_latency_stats)
from distributed_cluster_gpus_amd.configs.paper import \
    build_arrivals  # noqa: E402
from distributed_cluster_gpus_amd.engine.state import (  # noqa: E402
    alloc_state, engine_cfg, engine_dims)

from test_lat_bins_cpu import (LAST, LO, bits, edge_values, out,  # noqa: F401,E402
                               sweep_values)


def test_numpy_binning_agrees_with_the_header(out):  # noqa: F811
    rows, _ = out
    values = edge_values() + sweep_values()
    got = latency_bins(values)
    lo, hi = latency_bin_edges()
    for v, b in zip(values, got):
        hb, hlo, hhi = rows[bits(v)]
        assert b == hb and lo[b] == hlo and hi[b] == hhi, v
    h = latency_histogram(values)
    assert h.dtype == np.int64 and h.shape == (256,) and h.sum() == len(values)
    assert np.array_equal(h, np.bincount([rows[bits(v)][0] for v in values],
                                         minlength=256))


@pytest.mark.parametrize("n", [1, 5, 100, 12345])
def test_quantiles_hold_the_eighth_bound(n):
    rng = np.random.default_rng(n)
    x = np.sort(np.exp(rng.uniform(np.log(LO), np.log(LAST), n)))
    x = x[(x >= LO) & (x < LAST)]
    h = latency_histogram(x)
    for q in DEFAULT_QUANTILES:
        k = int(np.ceil(q * float(len(x))))
        v = float(latency_quantile(h, q))
        assert x[k - 1] < v <= 1.125 * x[k - 1], (q, x[k - 1], v)
    assert np.isnan(latency_quantile(np.zeros(256, np.int64), 0.5))
    top = np.zeros(256, np.int64)
    top[255] = 3
    assert latency_quantile(top, 0.5) == np.inf
    # leading axes are batch axes
    two = np.stack([h, np.zeros(256, np.int64)])
    v = latency_quantile(two, 0.99)
    assert v.shape == (2,) and np.isnan(v[1]) and v[0] == latency_quantile(h, 0.99)


def _stats_of(values, hist, names):
    """LatencyStats of per-replica figures values [n_row, 2, K, R] (NaN =
    the replica has none), by plain two-pass numpy."""
    some = ~np.isnan(values)
    n = some.sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(some, values, 0.0).sum(axis=-1) / n
        dx = np.where(some, values - mean[..., None], 0.0)
        m2 = (dx * dx).sum(axis=-1)
        lo = np.where(some, values, np.inf).min(axis=-1)
        hi = np.where(some, values, -np.inf).max(axis=-1)
    nan = np.full(n.shape, np.nan)
    st = np.stack([n.astype(np.float64), np.where(n > 0, mean, nan), m2,
                   np.where(n > 0, lo, nan), np.where(n > 0, hi, nan)], axis=-1)
    K = values.shape[2]
    return LatencyStats.from_tensor(hist, st, quantiles=[0.5] * (K - 2),
                                    dc_names=names, sla_s=0.5), \
        (dx * dx).max(axis=-1)


def test_merge_of_chunks_equals_the_whole():
    rng = np.random.default_rng(3)
    n_row, K, R = 3, 4, 50
    values = rng.lognormal(0.0, 1.0, (n_row, 2, K, R)) + 10.0
    values[rng.random(values.shape) < 0.2] = np.nan
    values[0, 0, 0, :] = np.nan          # a cell no replica has
    values[1, 1, 1, :20] = np.nan        # ... and one a whole chunk lacks
    hists = rng.integers(0, 1000, (R, n_row, 2, 256))
    names = ["a", "b", "ALL"]
    cuts = [0, 20, 21, 37, 50]
    parts = [_stats_of(values[..., a:b], hists[a:b].sum(axis=0), names)[0]
             for a, b in zip(cuts[:-1], cuts[1:])]
    whole, dev2 = _stats_of(values, hists.sum(axis=0), names)
    got = merge_latency_stats(parts)
    assert np.array_equal(got.pop_hist, whole.pop_hist)
    assert np.array_equal(got.n, whole.n) and got.n[0, 0, 0] == 0
    assert np.array_equal(got.min, whole.min, equal_nan=True)
    assert np.array_equal(got.max, whole.max, equal_nan=True)
    some = whole.n > 0
    assert np.array_equal(np.isnan(got.mean), ~some)
    assert np.allclose(got.mean[some], whole.mean[some], rtol=1e-12, atol=0.0)
    err = np.abs(got.m2 - whole.m2)
    assert (err <= 1e-9 * np.abs(whole.m2) + 1e-9 * whole.n * dev2).all()
    assert (got.m2[~some] == 0).all()
    assert got.metrics == ["p50", "p50", "sla_miss_frac", "jobs"]
    with pytest.raises(ValueError):
        merge_latency_stats([])
    # frames: one row per (dc, type, metric) / per non-empty bin
    df = latency_frame(got)
    assert list(df.columns) == ["dc", "type", "metric", "n", "mean", "std",
                                "stderr", "ci_lo", "ci_hi", "min", "max"]
    assert len(df) == n_row * 2 * K
    assert list(df["dc"][:2 * K]) == ["a"] * (2 * K)
    assert list(df["type"][:2 * K]) == ["inference"] * K + ["training"] * K
    row = df[(df.dc == "b") & (df.type == "training") &
             (df.metric == "sla_miss_frac")].iloc[0]
    v = values[1, 1, 2]
    v = v[~np.isnan(v)]
    assert row["n"] == len(v)
    assert np.isclose(row["std"], np.std(v, ddof=1), rtol=1e-9)
    hf = latency_hist_frame(got)
    assert list(hf.columns) == ["dc", "type", "bin_lo_s", "bin_hi_s", "count"]
    assert hf["count"].sum() == hists.sum() and (hf["count"] > 0).all()


def test_state_has_the_histograms_only_when_asked(paper_sc):
    sc = paper_sc
    R = 3
    dims = engine_dims(sc, algo="default_policy", n_rep=R, tcap=8, qcap=16,
                       latency_hist=True)
    t = alloc_state(dims, sc, "cpu")
    assert dims.lat_hist
    assert t["lh_hist"].shape == (R, sc.n_dc, 2, 256)
    assert t["lh_over"].shape == (R, sc.n_dc, 2)
    for k in ("lh_hist", "lh_over"):
        assert t[k].dtype == torch.int32 and not t[k].any()
    dims = engine_dims(sc, algo="default_policy", n_rep=R, tcap=8, qcap=16)
    t = alloc_state(dims, sc, "cpu")
    assert not dims.lat_hist
    assert "lh_hist" not in t and "lh_over" not in t


def test_cfg_carries_the_sla(paper_sc):
    sc = paper_sc
    inf, trn = build_arrivals()
    dims = engine_dims(sc, algo="default_policy", n_rep=2, tcap=8, qcap=16,
                       sla_p99_ms=250.0)
    assert engine_cfg(dims, sc, inf, trn)["lat_sla_s"] == 0.25
    dims = engine_dims(sc, algo="joint_nf", n_rep=2, tcap=8, qcap=16,
                       latency_hist=True, latency_sla_s=0.05)
    assert engine_cfg(dims, sc, inf, trn)["lat_sla_s"] == 0.05
    assert engine_cfg(engine_dims(sc, algo="joint_nf", n_rep=2, tcap=8,
                                  qcap=16), sc, inf, trn)["lat_sla_s"] == 0.5


def test_cli_flag_is_off_by_default():
    import run_sim
    assert run_sim.parse_args([]).latency_hist is False
    assert run_sim.parse_args(["--latency-hist"]).latency_hist is True


def _rank_stats(rank):
    """The deterministic LatencyStats of one of two replica groups."""
    rng = np.random.default_rng(11)
    values = rng.lognormal(0.0, 1.0, (3, 2, 6, 40)) + 1.0
    values[rng.random(values.shape) < 0.3] = np.nan
    hists = rng.integers(0, 2 ** 40, (40, 3, 2, 256))   # beyond i32, below 2^53
    sl = slice(0, 17) if rank == 0 else slice(17, 40)
    return _stats_of(values[..., sl], hists[sl].sum(axis=0), ["a", "b", "ALL"])[0]


def _worker_allgather(rank, world, port, q):
    import os
    import sys
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from distributed_cluster_gpus_amd.parallel.dist import \
            allgather_series_stats
        mine = _rank_stats(rank)
        parts = allgather_series_stats(torch.from_numpy(mine.to_flat()))
        merged = merge_latency_stats([
            LatencyStats.from_flat(p.numpy(), mine.quantiles, mine.dc_names,
                                   mine.sla_s) for p in parts])
        q.put((rank, merged.to_flat()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))


def test_flat_form_round_trips_and_merges_across_two_ranks():
    import torch.multiprocessing as mp
    a = _rank_stats(0)
    b = LatencyStats.from_flat(a.to_flat(), a.quantiles, a.dc_names, a.sla_s)
    assert np.array_equal(a.pop_hist, b.pop_hist) and a.pop_hist.max() > 2 ** 40
    assert np.array_equal(a.to_array(), b.to_array(), equal_nan=True)
    assert b.metrics == a.metrics and b.n.dtype == np.int64

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_allgather, args=(r, 2, 29861, q))
             for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    want = merge_latency_stats([_rank_stats(0), _rank_stats(1)]).to_flat()
    for rank in (0, 1):
        assert not isinstance(res[rank], str), f"rank {rank}: {res[rank]}"
        assert np.array_equal(res[rank], want, equal_nan=True), rank
