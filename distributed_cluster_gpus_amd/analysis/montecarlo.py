"""Monte-Carlo population statistics from a batched-engine run.

The scalar reference simulates ONE trajectory per run; the batched MI355X
engine advances thousands of replicas, so every output becomes a
DISTRIBUTION.  This module turns the engine's per-replica metric tensors into
a population report: mean / std / standard error / percentiles / confidence
intervals for energy, completed jobs and latency — the capability SURVEY §6
names as the rebuild's north star.
"""
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Sequence

import numpy as np
import pandas as pd

# normal-approximation z per confidence level (shared by every report here)
_Z_TABLE = {0.90: 1.6449, 0.95: 1.9600, 0.99: 2.5758}


def _z(confidence: float) -> float:
    return _Z_TABLE.get(round(confidence, 2), 1.9600)


def population_frame(engine) -> pd.DataFrame:
    """One row per replica with its headline outcomes."""
    t = engine.t
    jobs = t["jobs_done"].cpu().numpy().astype(np.float64)
    jobs_inf = t["jobs_done_inf"].cpu().numpy().astype(np.float64)
    energy = t["energy_j"].sum(dim=1).cpu().numpy()
    lat = t["sum_lat"].cpu().numpy()
    lat_inf = t["sum_lat_inf"].cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_lat = np.where(jobs > 0, lat / jobs, np.nan)
        mean_lat_inf = np.where(jobs_inf > 0, lat_inf / jobs_inf, np.nan)
    return pd.DataFrame({
        "replica": np.arange(len(jobs)) + engine.shard.start,
        "jobs_completed": jobs,
        "jobs_inference": jobs_inf,
        "total_energy_kJ": energy / 1e3,
        "mean_latency_s": mean_lat,
        "mean_inf_latency_ms": mean_lat_inf * 1e3,
        "events": t["ev_count"].cpu().numpy().astype(np.float64),
    })


def population_report(engine, out_dir: Optional[str] = None,
                      confidence: float = 0.95) -> Dict:
    """Population statistics dict (+ CSV/figure artifacts when out_dir set).

    Returns, per metric: mean, std (across replicas), standard error of the
    mean, the normal-approximation confidence interval, and percentiles —
    i.e. Monte-Carlo error bars on every simulator output.
    """
    df = population_frame(engine)
    z = _z(confidence)
    metrics = ["jobs_completed", "total_energy_kJ", "mean_latency_s",
               "mean_inf_latency_ms"]
    report: Dict = {"replicas": int(len(df)), "confidence": confidence}
    rows = []
    for m in metrics:
        v = df[m].dropna().values
        if len(v) == 0:
            continue
        mean, std = float(np.mean(v)), float(np.std(v, ddof=1)) if len(v) > 1 else 0.0
        se = std / np.sqrt(len(v)) if len(v) > 1 else 0.0
        entry = {
            "metric": m, "mean": mean, "std": std, "stderr": se,
            "ci_lo": mean - z * se, "ci_hi": mean + z * se,
            "p01": float(np.percentile(v, 1)), "p50": float(np.percentile(v, 50)),
            "p99": float(np.percentile(v, 99)),
        }
        rows.append(entry)
        report[m] = entry
    if out_dir is not None:
        import os

        from .render import emit
        os.makedirs(out_dir, exist_ok=True)
        df.to_csv(os.path.join(out_dir, "population.csv"), index=False)
        pd.DataFrame(rows).to_csv(os.path.join(out_dir, "population_stats.csv"),
                                  index=False)
        emit(df[["total_energy_kJ"]], out_dir, "population_energy_hist",
             kind="hist", y="total_energy_kJ",
             title=f"Total energy across {len(df)} replicas")
        emit(df[["jobs_completed"]], out_dir, "population_jobs_hist",
             kind="hist", y="jobs_completed",
             title=f"Completed jobs across {len(df)} replicas")
    return report


# ---------------------------------------------------------------------------
# Population TIME SERIES: per-tick statistics over the replica ensemble
# (BatchedEngine(pop_series=True); reduced on the GPU by ops reduce_series)
# ---------------------------------------------------------------------------
@dataclass
class Moments:
    """{n, mean, M2, min, max} of a per-replica figure over a replica
    ensemble, per cell: ``n`` (int64), ``mean``, ``m2`` (sum of squared
    deviations from the mean), ``min`` and ``max`` share one shape.  Cells
    with n == 0 hold NaN mean/min/max and m2 == 0."""
    n: np.ndarray
    mean: np.ndarray
    m2: np.ndarray
    min: np.ndarray
    max: np.ndarray

    @classmethod
    def from_array(cls, a, **own):
        """a: [..., 5] = {n, mean, M2, min, max}; ``own``: the fields a
        subclass adds."""
        a = np.asarray(a, dtype=np.float64)
        return cls(a[..., 0].astype(np.int64), a[..., 1].copy(),
                   a[..., 2].copy(), a[..., 3].copy(), a[..., 4].copy(),
                   **own)

    def to_array(self) -> np.ndarray:
        """Inverse of from_array: [..., 5] float64."""
        return np.stack([self.n.astype(np.float64), self.mean, self.m2,
                         self.min, self.max], axis=-1)

    @classmethod
    def from_values(cls, values, slices, **own):
        """values: [R, K] per-replica figures; slices: one ``(a, b)`` replica
        range per group (empty where this rank holds none of it).  Two-pass,
        shifted by the mean: sum of (x - mean)^2.  NaN figures are skipped."""
        v = np.asarray(values, dtype=np.float64)
        G, K = len(slices), v.shape[1]
        n = np.zeros((G, K), np.int64)
        mean, lo, hi = (np.full((G, K), np.nan) for _ in range(3))
        m2 = np.zeros((G, K))
        for g, (a, b) in enumerate(slices):
            for k in range(K):
                x = v[a:b, k]
                x = x[~np.isnan(x)]
                if x.size == 0:
                    continue
                mu = x.sum() / x.size
                d = x - mu
                n[g, k], mean[g, k] = x.size, mu
                m2[g, k] = (d * d).sum()
                lo[g, k], hi[g, k] = x.min(), x.max()
        return cls(n, mean, m2, lo, hi, **own)

    def merge(self, b, **own):
        """Statistics of the union of two disjoint replica groups: Chan et
        al. parallel combination of (n, mean, M2) per cell, min and max
        directly.  An empty side contributes nothing (its NaN mean never
        enters the arithmetic).  The other fields are ``self``'s, or
        ``own``'s."""
        a = self
        na, nb = a.n.astype(np.float64), b.n.astype(np.float64)
        n = na + nb
        ea, eb = a.n == 0, b.n == 0
        ma, mb = np.where(ea, 0.0, a.mean), np.where(eb, 0.0, b.mean)
        delta = mb - ma
        safe_n = np.where(n > 0, n, 1.0)
        mean = ma + delta * (nb / safe_n)
        m2 = a.m2 + b.m2 + delta * delta * (na * nb / safe_n)
        return replace(
            a, n=a.n + b.n,
            mean=np.where(ea, b.mean, np.where(eb, a.mean, mean)),
            m2=np.where(ea, b.m2, np.where(eb, a.m2, m2)),
            min=np.fmin(a.min, b.min), max=np.fmax(a.max, b.max), **own)

    def std(self) -> np.ndarray:
        """Sample standard deviation (ddof=1); 0 where n < 2."""
        multi = self.n > 1
        return np.where(multi, np.sqrt(np.maximum(self.m2, 0.0)
                                       / np.where(multi, self.n - 1, 1)), 0.0)

    def stderr(self) -> np.ndarray:
        """Standard error of the mean; 0 where n < 2."""
        multi = self.n > 1
        return np.where(multi, self.std()
                        / np.sqrt(np.where(multi, self.n, 1)), 0.0)


def _tree_merge(parts, cls, name: str):
    """Pairwise (tree-order) ``merge`` of a non-empty sequence."""
    parts = list(parts)
    if not parts:
        raise ValueError(f"{name} needs at least one {cls.__name__}")
    while len(parts) > 1:
        nxt = [parts[i].merge(parts[i + 1])
               for i in range(0, len(parts) - 1, 2)]
        if len(parts) % 2:
            nxt.append(parts[-1])
        parts = nxt
    return parts[0]


@dataclass
class SeriesStats(Moments):
    """Per-tick ensemble statistics.  ``time`` is [T]; the moments are
    [T, len(dc_names), len(metrics)].  The last entry of ``dc_names`` is the
    fleet row."""
    time: np.ndarray
    metrics: List[str]
    dc_names: List[str]

    @classmethod
    def from_tensor(cls, stats, time, metrics, dc_names) -> "SeriesStats":
        """stats: [T, n_row, K, 5] = {n, mean, M2, min, max} (tensor or array,
        on the host), time: [T]."""
        return cls.from_array(
            stats, time=np.asarray(time, dtype=np.float64).copy(),
            metrics=list(metrics), dc_names=list(dc_names))

    def _reached(self) -> np.ndarray:
        """[T] bool: the ticks at least one replica has reached."""
        T = len(self.time)
        return self.n.reshape(T, -1).max(axis=1) > 0 if self.n.size \
            else np.zeros(T, bool)

    def trimmed(self) -> "SeriesStats":
        """Drop the ticks no replica has reached."""
        keep = self._reached()
        return replace(self, time=self.time[keep], n=self.n[keep],
                       mean=self.mean[keep], m2=self.m2[keep],
                       min=self.min[keep], max=self.max[keep])

    def _padded(self, T: int) -> "SeriesStats":
        """Extend to T ticks with empty cells (n = 0)."""
        extra = T - len(self.time)
        if extra <= 0:
            return self
        shape = (extra,) + self.n.shape[1:]
        nan = np.full(shape, np.nan)
        return replace(
            self, time=np.concatenate([self.time, np.full(extra, np.nan)]),
            n=np.concatenate([self.n, np.zeros(shape, np.int64)]),
            mean=np.concatenate([self.mean, nan]),
            m2=np.concatenate([self.m2, np.zeros(shape)]),
            min=np.concatenate([self.min, nan]),
            max=np.concatenate([self.max, nan]))

    def merge(self, b: "SeriesStats") -> "SeriesStats":
        assert self.metrics == b.metrics and self.dc_names == b.dc_names
        T = max(len(self.time), len(b.time))
        a, b = self._padded(T), b._padded(T)
        # a tick's time comes from whichever side has reached it
        return Moments.merge(a, b,
                             time=np.where(a._reached(), a.time, b.time))


def merge_series_stats(parts: Sequence[SeriesStats]) -> SeriesStats:
    """Combine the statistics of disjoint replica groups (shards, ranks,
    separate runs) into those of their union: pairwise (tree-order)
    ``Moments.merge``."""
    return _tree_merge(parts, SeriesStats, "merge_series_stats")


SERIES_COLUMNS = ["time_s", "dc", "metric", "n", "mean", "std", "stderr",
                  "ci_lo", "ci_hi", "min", "max"]


def series_frame(stats: SeriesStats, confidence: float = 0.95) -> pd.DataFrame:
    """Long-form rows (tick-major, then DC, then metric) with the sample
    standard deviation (ddof=1), the standard error of the mean and the
    normal-approximation confidence interval; zero width when n < 2."""
    z = _z(confidence)
    T, D, K = len(stats.time), len(stats.dc_names), len(stats.metrics)
    n = stats.n.reshape(-1)
    mean = stats.mean.reshape(-1)
    std, se = stats.std().reshape(-1), stats.stderr().reshape(-1)
    return pd.DataFrame({
        "time_s": np.repeat(stats.time, D * K),
        "dc": np.tile(np.repeat(np.asarray(stats.dc_names, object), K), T),
        "metric": np.tile(np.asarray(stats.metrics, object), T * D),
        "n": n, "mean": mean, "std": std, "stderr": se,
        "ci_lo": mean - z * se, "ci_hi": mean + z * se,
        "min": stats.min.reshape(-1), "max": stats.max.reshape(-1),
    }, columns=SERIES_COLUMNS)


def population_series_report(engine, out_dir: str,
                             confidence: float = 0.95) -> pd.DataFrame:
    """Write population_series.csv (schema: docs/log_format.md) and two
    figures: fleet power mean +- CI over time, per-DC queue length mean over
    time.  Returns the long-form frame."""
    import os

    from .render import emit
    stats = engine.population_series()
    df = series_frame(stats, confidence)
    os.makedirs(out_dir, exist_ok=True)
    df.to_csv(os.path.join(out_dir, "population_series.csv"), index=False)
    fleet = stats.dc_names[-1]
    power = df[(df["dc"] == fleet) & (df["metric"] == "power_w")]
    emit(power[["time_s", "mean", "ci_lo", "ci_hi", "n"]], out_dir,
         "population_series_fleet_power", kind="band", x="time_s", y="mean",
         title=f"Fleet power, mean and {confidence:.0%} CI over replicas",
         ylabel="W")
    q = df[(df["dc"] != fleet) & df["metric"].isin(["q_inf", "q_trn"])]
    # means add: E[q_inf + q_trn] = E[q_inf] + E[q_trn]
    q = q.groupby(["time_s", "dc"], sort=False, as_index=False)["mean"].sum() \
        .rename(columns={"mean": "queue_len_mean"})
    emit(q, out_dir, "population_series_queue_len", kind="line", x="time_s",
         y="queue_len_mean", hue="dc",
         title="Queue length per DC, mean over replicas", ylabel="jobs")
    return df


# ---------------------------------------------------------------------------
# Latency distribution: per-replica histograms of the job sojourn
# (BatchedEngine(latency_hist=True); reduced on the GPU by ops latency_reduce)
# ---------------------------------------------------------------------------
# The bins of ops/csrc/hip/lat_bins.hpp, restated in numpy: exponent and top 3
# mantissa bits of the f64 pattern, 8 bins per octave from 2^-14 s to 2^18 s.
LH_BINS = 256
_LH_SHIFT = 49
_LH_KEY0 = (1023 - 14) << 3
JOB_TYPES = ["inference", "training"]
DEFAULT_QUANTILES = (0.5, 0.9, 0.99, 0.999)


def latency_bin_edges():
    """(lower[256], upper[256]) in seconds.  Bin b holds lower <= x < upper;
    bin 0 also everything below, bin 255 everything above (upper = +inf)."""
    keys = (np.arange(LH_BINS + 1, dtype=np.uint64) + np.uint64(_LH_KEY0)) \
        << np.uint64(_LH_SHIFT)
    edges = keys.view(np.float64).copy()
    upper = edges[1:].copy()
    upper[-1] = np.inf
    return edges[:-1], upper


def latency_bins(latencies) -> np.ndarray:
    """Bin index of each sojourn (seconds); negatives and NaN count as 0."""
    x = np.ascontiguousarray(latencies, dtype=np.float64)
    x = np.where(x > 0.0, x, 0.0)
    key = (x.view(np.uint64) >> np.uint64(_LH_SHIFT)).astype(np.int64)
    return np.clip(key - _LH_KEY0, 0, LH_BINS - 1)


def latency_histogram(latencies) -> np.ndarray:
    """int64[256] histogram of sojourns in the engine's bins, so that the
    ``latency_s`` column of a scalar engine's job_log.csv yields the same
    report as the batched engine's in-kernel histograms."""
    return np.bincount(latency_bins(latencies).reshape(-1),
                       minlength=LH_BINS).astype(np.int64)


def latency_quantile(pop_hist, q: float) -> np.ndarray:
    """Quantile q of histograms [..., 256]: the upper edge of the first bin
    whose cumulative count reaches ceil(q * n); NaN where n == 0.  The true
    order statistic x of that rank satisfies x < reported <= 1.125 * x
    whenever 2^-14 <= x < 1.875 * 2^17 seconds."""
    h = np.asarray(pop_hist, dtype=np.int64)
    cum = np.cumsum(h, axis=-1)
    n = cum[..., -1]
    rank = np.ceil(q * n.astype(np.float64)).astype(np.int64)
    b = (cum < rank[..., None]).sum(axis=-1)
    upper = latency_bin_edges()[1]
    return np.where(n > 0, upper[np.minimum(b, LH_BINS - 1)], np.nan)


def quantile_label(q: float) -> str:
    return f"p{q * 100:.6g}"


@dataclass
class LatencyStats(Moments):
    """Latency distribution over the replica ensemble.  ``pop_hist`` is
    [len(dc_names), 2, 256] int64, the histogram pooled over the replicas;
    the moments are [len(dc_names), 2, len(metrics)]: statistics of each
    per-replica figure over the replicas that have one (a replica with no
    finished job in a cell has no quantile and no SLA-miss fraction there).
    ``metrics`` is one label per quantile, then ``sla_miss_frac`` and
    ``jobs``.  The last entry of ``dc_names`` is the fleet row."""
    pop_hist: np.ndarray
    quantiles: List[float]
    metrics: List[str]
    dc_names: List[str]
    job_types: List[str]
    bin_lo: np.ndarray
    bin_hi: np.ndarray
    sla_s: float

    @classmethod
    def from_tensor(cls, pop_hist, stats, quantiles, dc_names,
                    sla_s) -> "LatencyStats":
        """pop_hist: [n_row, 2, 256], stats: [n_row, 2, Q + 2, 5] = {n, mean,
        M2, min, max} (tensors or arrays, on the host)."""
        lo, hi = latency_bin_edges()
        qs = [float(q) for q in quantiles]
        return cls.from_array(
            stats, pop_hist=np.asarray(pop_hist).astype(np.int64),
            quantiles=qs, metrics=[quantile_label(q) for q in qs] +
            ["sla_miss_frac", "jobs"],
            dc_names=list(dc_names), job_types=list(JOB_TYPES),
            bin_lo=lo, bin_hi=hi, sla_s=float(sla_s))

    def to_flat(self) -> np.ndarray:
        """Histogram and statistics as one f64 vector, the form that travels
        between ranks; counts are exact below 2^53."""
        return np.concatenate([self.pop_hist.astype(np.float64).reshape(-1),
                               self.to_array().reshape(-1)])

    @classmethod
    def from_flat(cls, flat, quantiles, dc_names, sla_s) -> "LatencyStats":
        """Inverse of to_flat."""
        flat = np.asarray(flat, dtype=np.float64)
        n_row, K = len(dc_names), len(quantiles) + 2
        n_pop = n_row * 2 * LH_BINS
        return cls.from_tensor(
            flat[:n_pop].astype(np.int64).reshape(n_row, 2, LH_BINS),
            flat[n_pop:].reshape(n_row, 2, K, 5), quantiles, dc_names, sla_s)

    def pooled_quantile(self, q: float) -> np.ndarray:
        """[n_row, 2]: quantile q of the pooled histogram."""
        return latency_quantile(self.pop_hist, q)

    def merge(self, b: "LatencyStats") -> "LatencyStats":
        assert self.quantiles == b.quantiles and \
            self.dc_names == b.dc_names and self.sla_s == b.sla_s
        return Moments.merge(self, b, pop_hist=self.pop_hist + b.pop_hist)


def merge_latency_stats(parts: Sequence[LatencyStats]) -> LatencyStats:
    """Combine disjoint replica groups (shards, ranks, separate runs):
    histograms add; the moments merge as in merge_series_stats, in the same
    tree order."""
    return _tree_merge(parts, LatencyStats, "merge_latency_stats")


LATENCY_COLUMNS = ["dc", "type", "metric", "n", "mean", "std", "stderr",
                   "ci_lo", "ci_hi", "min", "max"]
LATENCY_HIST_COLUMNS = ["dc", "type", "bin_lo_s", "bin_hi_s", "count"]


def latency_frame(stats: LatencyStats, confidence: float = 0.95) -> pd.DataFrame:
    """Long-form rows (DC, then job type, then metric) with the sample
    standard deviation (ddof=1), the standard error of the mean and the
    normal-approximation confidence interval over the replicas; zero width
    when n < 2."""
    z = _z(confidence)
    D, J, K = len(stats.dc_names), len(stats.job_types), len(stats.metrics)
    n = stats.n.reshape(-1)
    mean = stats.mean.reshape(-1)
    std, se = stats.std().reshape(-1), stats.stderr().reshape(-1)
    return pd.DataFrame({
        "dc": np.repeat(np.asarray(stats.dc_names, object), J * K),
        "type": np.tile(np.repeat(np.asarray(stats.job_types, object), K), D),
        "metric": np.tile(np.asarray(stats.metrics, object), D * J),
        "n": n, "mean": mean, "std": std, "stderr": se,
        "ci_lo": mean - z * se, "ci_hi": mean + z * se,
        "min": stats.min.reshape(-1), "max": stats.max.reshape(-1),
    }, columns=LATENCY_COLUMNS)


def latency_hist_frame(stats: LatencyStats) -> pd.DataFrame:
    """The pooled histogram, one row per non-empty (DC, job type, bin)."""
    d, j, b = np.nonzero(stats.pop_hist)
    return pd.DataFrame({
        "dc": np.asarray(stats.dc_names, object)[d],
        "type": np.asarray(stats.job_types, object)[j],
        "bin_lo_s": stats.bin_lo[b], "bin_hi_s": stats.bin_hi[b],
        "count": stats.pop_hist[d, j, b],
    }, columns=LATENCY_HIST_COLUMNS)


def latency_report(engine, out_dir: str, quantiles=DEFAULT_QUANTILES,
                   confidence: float = 0.95, logger=None) -> pd.DataFrame:
    """Write latency_quantiles.csv and latency_hist.csv (schema:
    docs/log_format.md) and log, per job type, the fleet's pooled p99 against
    the SLA.  Returns the long-form quantile frame."""
    import logging
    import os

    from ..utils.logging import LOGGER_NAME
    stats = engine.latency_distribution(quantiles)
    df = latency_frame(stats, confidence)
    os.makedirs(out_dir, exist_ok=True)
    df.to_csv(os.path.join(out_dir, "latency_quantiles.csv"), index=False)
    latency_hist_frame(stats).to_csv(
        os.path.join(out_dir, "latency_hist.csv"), index=False)
    log = logger or logging.getLogger(LOGGER_NAME)
    p99 = stats.pooled_quantile(0.99)[-1]
    jobs = stats.pop_hist[-1].sum(axis=-1)
    for j, name in enumerate(stats.job_types):
        verdict = "no jobs" if jobs[j] == 0 else \
            ("within" if p99[j] <= stats.sla_s else "MISSES")
        log.info(f"latency_hist: {name} pooled p99 <= {p99[j]:.4g} s over "
                 f"{int(jobs[j])} jobs, SLA {stats.sla_s:g} s: {verdict}")
    return df


# ---------------------------------------------------------------------------
# Parameter sweeps: per-group statistics of the headline outcomes
# (BatchedEngine(sweep=Sweep); engine/sweep.py)
# ---------------------------------------------------------------------------
SWEEP_METRICS = ["total_energy_j", "jobs", "jobs_inf", "mean_latency_s",
                 "mean_inf_latency_s", "mean_wait_s", "events"]


def sweep_replica_metrics(t) -> np.ndarray:
    """[R, len(SWEEP_METRICS)] f64 from the host copies of the engine's
    metric tensors.  A replica without a finished (inference) job has no mean
    latency or wait: NaN there."""
    jobs = np.asarray(t["jobs_done"], dtype=np.float64)
    jobs_inf = np.asarray(t["jobs_done_inf"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cols = [
            np.asarray(t["energy_j"], dtype=np.float64).sum(axis=1),
            jobs, jobs_inf,
            np.where(jobs > 0, np.asarray(t["sum_lat"]) / jobs, np.nan),
            np.where(jobs_inf > 0, np.asarray(t["sum_lat_inf"]) / jobs_inf,
                     np.nan),
            np.where(jobs > 0, np.asarray(t["sum_wait"]) / jobs, np.nan),
            np.asarray(t["ev_count"], dtype=np.float64),
        ]
    return np.stack(cols, axis=1)


@dataclass
class SweepStats(Moments):
    """Per-group ensemble statistics of a sweep: the moments are [G,
    len(metrics)], each over the group's replicas that have the figure (NaN
    cells are skipped, as in LatencyStats).  ``metrics`` defaults to
    SWEEP_METRICS."""
    metrics: Optional[List[str]] = None

    def __post_init__(self):
        self.metrics = list(SWEEP_METRICS if self.metrics is None
                            else self.metrics)

    def merge(self, b: "SweepStats") -> "SweepStats":
        assert self.metrics == b.metrics and self.n.shape == b.n.shape
        return Moments.merge(self, b)


def merge_sweep_stats(parts: Sequence[SweepStats]) -> SweepStats:
    """Combine the per-group statistics of disjoint replica sets (shards,
    ranks, separate runs of one sweep): ``Moments.merge`` per group and
    metric, in the tree order of merge_series_stats."""
    return _tree_merge(parts, SweepStats, "merge_sweep_stats")


SWEEP_STAT_COLUMNS = ["n", "mean", "stderr", "ci_lo", "ci_hi"]


def sweep_frame(stats: SweepStats, sweep, confidence: float = 0.95,
                base=None) -> pd.DataFrame:
    """One row per group: ``group``, its parameters (``sweep.frame``), then
    ``<metric>_n / _mean / _stderr / _ci_lo / _ci_hi`` per metric, with the
    normal-approximation confidence interval over the group's replicas; zero
    width when n < 2."""
    z = _z(confidence)
    df = sweep.frame(base)
    if len(df) != stats.n.shape[0]:
        raise ValueError(f"sweep has {len(df)} groups, the statistics "
                         f"{stats.n.shape[0]}")
    se = stats.stderr()
    for k, m in enumerate(stats.metrics):
        df[f"{m}_n"] = stats.n[:, k]
        df[f"{m}_mean"] = stats.mean[:, k]
        df[f"{m}_stderr"] = se[:, k]
        df[f"{m}_ci_lo"] = stats.mean[:, k] - z * se[:, k]
        df[f"{m}_ci_hi"] = stats.mean[:, k] + z * se[:, k]
    return df


def sweep_report(engine, out_dir: str, confidence: float = 0.95,
                 quantiles=DEFAULT_QUANTILES) -> pd.DataFrame:
    """Write ``population/sweep.csv`` under ``out_dir``: one row per group
    (``sweep_frame``); with ``latency_hist`` on also the group's pooled fleet
    quantiles and mean SLA-miss fraction per job type; and one figure, energy
    against the sweep's first axis.  Per-group latency columns come from this
    rank's replicas.  Returns the frame."""
    import os

    from .render import emit
    sweep = engine.sweep
    df = sweep_frame(engine.sweep_stats(), sweep, confidence,
                     engine.sweep_base)
    if engine.dims.lat_hist:
        cols = {}
        for g in range(sweep.n_groups):
            a, b = sweep.slice_of(g, engine.shard)
            ls = engine.latency_distribution(quantiles, group=g) \
                if b > a else None
            for j, jt in enumerate(JOB_TYPES):
                for q in quantiles:
                    cols.setdefault(f"{jt}_{quantile_label(q)}_s", []).append(
                        ls.pooled_quantile(q)[-1, j] if ls else np.nan)
                k = len(quantiles)   # sla_miss_frac follows the quantiles
                cols.setdefault(f"{jt}_sla_miss_frac", []).append(
                    ls.mean[-1, j, k] if ls else np.nan)
        for name, col in cols.items():
            df[name] = col
    pop_dir = os.path.join(out_dir, "population")
    os.makedirs(pop_dir, exist_ok=True)
    df.to_csv(os.path.join(pop_dir, "sweep.csv"), index=False)
    axis = sweep.axes[0]
    rest = [a for a in sweep.axes[1:]]
    fig = df[[axis, "total_energy_j_mean", "total_energy_j_ci_lo",
              "total_energy_j_ci_hi"] + rest].rename(columns={
                  "total_energy_j_mean": "mean",
                  "total_energy_j_ci_lo": "ci_lo",
                  "total_energy_j_ci_hi": "ci_hi"})
    hue = None
    if rest:
        fig["point"] = fig[rest].astype(str).agg(", ".join, axis=1)
        hue = "point"
    emit(fig, pop_dir, f"sweep_energy_vs_{axis}", kind="band", x=axis,
         y="mean", hue=hue, ylabel="J",
         title=f"Energy per replica against {axis}, mean and "
               f"{confidence:.0%} CI per group")
    return df
