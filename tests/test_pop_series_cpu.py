"""Population time-series statistics, host side (no GPU): the Chan merge of
per-group (n, mean, M2, min, max), the long-form frame, and the cross-rank
all-gather (gloo, world_size 2).

Tolerances are f64 epsilon (2.2e-16) times the term count with a wide margin,
not measured: a mean over <= 1e3 terms is good to ~1e-13 relative; M2 is a sum
of n squares, each carrying the mean's absolute error against deviations of
order max|x - mean|, hence the atol term.  What the f64 representation of a
1e9-sized mean adds is worked out where the chunk sizes are chosen."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T, D, K = 3, 4, 5
METRICS = [f"m{k}" for k in range(K)]
DCS = [f"dc{d}" for d in range(D - 1)] + ["ALL"]


def _values(rng, n):
    """[n, T, D, K] samples; metric 0 is the ill-conditioned 1e9 + N(0,1)
    column (energy-like), the rest O(1)..O(1e3) with offsets that keep their
    means away from zero (a mean that cancels to ~0 has no relative accuracy
    to speak of)."""
    x = rng.normal(size=(n, T, D, K)) * np.array([1.0, 3.0, 50.0, 0.1, 1e3])
    return x + np.array([1e9, 10.0, -200.0, 0.5, 5e3])


def _stats_of(x, present):
    """SeriesStats of samples x [n, T, D, K] where replica i has reached tick
    t iff present[i, t] — plain numpy, per tick."""
    from distributed_cluster_gpus_amd.analysis.montecarlo import SeriesStats
    arr = np.zeros((T, D, K, 5))
    for t in range(T):
        v = x[present[:, t], t]
        arr[t, ..., 0] = len(v)
        if len(v):
            m = v.mean(axis=0)
            arr[t, ..., 1] = m
            arr[t, ..., 2] = ((v - m) ** 2).sum(axis=0)
            arr[t, ..., 3] = v.min(axis=0)
            arr[t, ..., 4] = v.max(axis=0)
        else:
            arr[t, ..., 1] = arr[t, ..., 3] = arr[t, ..., 4] = np.nan
    return SeriesStats.from_tensor(arr, np.arange(1, T + 1) * 5.0,
                                   METRICS, DCS)


# Per-tick chunk sizes.  The 1e9 column decides them: a mean near 1e9 is
# stored to ulp(1e9) = 1.2e-7 at best, and Chan's cross term
# nA*nB/n * delta^2 inherits 2*|delta|*nA*nB/n times that error whatever the
# merge does.  With one chunk of a single sample (its mean is exact,
# nA*nB/n < 1, |delta| <= max|x - mean| =: dev) the error is <= 2.4e-7 * dev,
# which the atol 1e-9 * n * dev^2 covers once n * dev >= 240; n = 1000 normal
# samples (dev >= 3) leave a factor of 12.  Each tick has one chunk of 1000,
# one empty and one single, in a different order.
COUNTS = np.array([[1000, 0, 1], [0, 1, 1000], [1, 1000, 0]])
# two sizeable chunks per tick (plus a small one): nA*nB/n grows with n, so
# the 1e9 column needs the bound written out in the test that uses these
COUNTS_SIZEABLE = np.array([[40, 17, 5], [23, 64, 9], [1, 3, 11]])


def _chunks(counts=COUNTS, seed=0):
    """Three chunks; counts[i, t] replicas of chunk i have reached tick t."""
    rng = np.random.default_rng(seed)
    xs, ps = [], []
    for c in counts:
        n = int(c.max())
        x = _values(rng, n)
        present = np.arange(n)[:, None] < c[None, :]
        xs.append(x)
        ps.append(present)
    return xs, ps


def _check_against(got, ref, x_all, p_all):
    """n/min/max exact; mean rtol 1e-12; M2 rtol 1e-9 + atol
    1e-9 * n * max|x - mean|^2."""
    assert np.array_equal(got.n, ref.n)
    assert np.array_equal(got.min, ref.min, equal_nan=True)
    assert np.array_equal(got.max, ref.max, equal_nan=True)
    np.testing.assert_allclose(got.mean, ref.mean, rtol=1e-12, atol=0.0)
    for t in range(T):
        v = x_all[p_all[:, t], t]
        dev2 = (np.abs(v - ref.mean[t]) ** 2).max(axis=0) if len(v) else 0.0
        atol = 1e-9 * ref.n[t] * dev2
        err = np.abs(got.m2[t] - ref.m2[t])
        assert (err <= 1e-9 * np.abs(ref.m2[t]) + atol).all(), (t, err.max())


def test_merge_matches_numpy_on_concatenation():
    from distributed_cluster_gpus_amd.analysis.montecarlo import \
        merge_series_stats
    xs, ps = _chunks()
    parts = [_stats_of(x, p) for x, p in zip(xs, ps)]
    assert (parts[1].n[0] == 0).all() and (parts[2].n[0] == 1).all()
    assert (parts[0].n[0] == 1000).all()
    x_all, p_all = np.concatenate(xs), np.concatenate(ps)
    ref = _stats_of(x_all, p_all)
    got = merge_series_stats(parts)
    _check_against(got, ref, x_all, p_all)
    assert got.metrics == METRICS and got.dc_names == DCS
    assert np.array_equal(got.time, ref.time)
    # an empty partner changes nothing, bit for bit
    alone = merge_series_stats([parts[0], _stats_of(xs[0][:0], ps[0][:0])])
    for f in ("n", "mean", "m2", "min", "max"):
        assert np.array_equal(getattr(alone, f), getattr(parts[0], f),
                              equal_nan=True), f


def test_merge_sizeable_chunks():
    """Two and three sizeable chunks per tick.  The well-conditioned columns
    keep the tolerances above.  For the 1e9 column the merged M2 can be no
    better than its inputs: each chunk mean is off by up to ~2 ulp(1e9)
    (rounding of the sum and of the quotient), so each pairwise step adds up
    to 2 * |delta| * nA*nB/n * 4 ulp; |delta| <= 2 dev and nA*nB/n <= n/4
    give atol = 4 * n * dev * ulp(1e9) over the two steps."""
    from distributed_cluster_gpus_amd.analysis.montecarlo import \
        merge_series_stats
    xs, ps = _chunks(COUNTS_SIZEABLE, seed=3)
    x_all, p_all = np.concatenate(xs), np.concatenate(ps)
    ref = _stats_of(x_all, p_all)
    got = merge_series_stats([_stats_of(x, p) for x, p in zip(xs, ps)])
    assert np.array_equal(got.n, ref.n)
    assert np.array_equal(got.min, ref.min) and np.array_equal(got.max, ref.max)
    np.testing.assert_allclose(got.mean, ref.mean, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got.m2[..., 1:], ref.m2[..., 1:], rtol=1e-9,
                               atol=0.0)
    ulp = np.spacing(1e9)
    for t in range(T):
        v = x_all[p_all[:, t], t, :, 0]
        dev = np.abs(v - ref.mean[t, :, 0]).max(axis=0)
        err = np.abs(got.m2[t, :, 0] - ref.m2[t, :, 0])
        assert (err <= 4 * len(v) * dev * ulp).all(), (t, err)


def test_series_frame_columns_and_intervals():
    from distributed_cluster_gpus_amd.analysis.montecarlo import series_frame
    xs, ps = _chunks(np.array([[1, 0, 11]] * 3), seed=1)
    st = _stats_of(xs[2], ps[2])      # per-tick n = 1, 0, 11
    df = series_frame(st, confidence=0.95)
    assert list(df.columns) == ["time_s", "dc", "metric", "n", "mean", "std",
                                "stderr", "ci_lo", "ci_hi", "min", "max"]
    assert len(df) == T * D * K
    # tick-major, then DC, then metric
    assert list(df["dc"][:K]) == [DCS[0]] * K
    assert list(df["metric"][:K]) == METRICS
    assert (df["time_s"][:D * K] == 5.0).all()
    full = df[df["n"] == 11]
    assert len(full) == D * K
    m2 = st.m2[2].reshape(-1)
    np.testing.assert_allclose(full["std"], np.sqrt(m2 / 10), rtol=1e-15)
    np.testing.assert_allclose(full["stderr"], full["std"] / np.sqrt(11),
                               rtol=1e-15)
    np.testing.assert_allclose(full["ci_hi"] - full["mean"],
                               1.96 * full["stderr"], rtol=1e-6)
    np.testing.assert_allclose(full["mean"] - full["ci_lo"],
                               1.96 * full["stderr"], rtol=1e-6)
    # the z-table of population_report
    wide = series_frame(st, confidence=0.99)
    w = wide[wide["n"] == 11]
    np.testing.assert_allclose(w["ci_hi"] - w["mean"], 2.5758 * w["stderr"],
                               rtol=1e-6)
    # n = 1: zero width, nothing undefined
    one = df[df["n"] == 1]
    assert len(one) == D * K
    assert (one["std"] == 0).all() and (one["stderr"] == 0).all()
    assert (one["ci_lo"] == one["mean"]).all()
    assert (one["ci_hi"] == one["mean"]).all()
    assert not one[["ci_lo", "ci_hi"]].isna().any().any()


def _worker_allgather(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    sys.path.insert(0, REPO)
    try:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from distributed_cluster_gpus_amd.analysis.montecarlo import (
            SeriesStats, merge_series_stats)
        from distributed_cluster_gpus_amd.parallel.dist import \
            allgather_series_stats
        xs, ps = _chunks(COUNTS_SIZEABLE, seed=7)
        mine = _stats_of(xs[rank * 2], ps[rank * 2])   # chunks 0 and 2
        flat = torch.from_numpy(mine.to_array()).reshape(-1)
        parts = allgather_series_stats(flat)
        assert len(parts) == world
        merged = merge_series_stats([
            SeriesStats.from_tensor(p.reshape(T, D, K, 5), mine.time,
                                    METRICS, DCS) for p in parts])
        q.put((rank, merged.to_array()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))


def test_allgather_series_stats_two_ranks():
    from distributed_cluster_gpus_amd.analysis.montecarlo import \
        merge_series_stats
    from distributed_cluster_gpus_amd.parallel.dist import \
        allgather_series_stats
    # not initialised: a no-op returning the input
    x = torch.arange(6, dtype=torch.float64)
    out = allgather_series_stats(x)
    assert len(out) == 1 and out[0] is x

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_allgather, args=(r, 2, 29853, q))
             for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    xs, ps = _chunks(COUNTS_SIZEABLE, seed=7)
    want = merge_series_stats([_stats_of(xs[0], ps[0]),
                               _stats_of(xs[2], ps[2])]).to_array()
    for rank in (0, 1):
        assert not isinstance(res[rank], str), f"rank {rank}: {res[rank]}"
        assert np.array_equal(res[rank], want, equal_nan=True), rank
