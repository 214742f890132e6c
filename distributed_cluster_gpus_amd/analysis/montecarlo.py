"""Monte-Carlo population statistics from a batched-engine run.

The scalar reference simulates ONE trajectory per run; the batched MI355X
engine advances thousands of replicas, so every output becomes a
DISTRIBUTION.  This module turns the engine's per-replica metric tensors into
a population report: mean / std / standard error / percentiles / confidence
intervals for energy, completed jobs and latency — the capability SURVEY §6
names as the rebuild's north star.
"""
from dataclasses import dataclass
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
class SeriesStats:
    """Per-tick ensemble statistics.  ``time`` is [T]; ``n``, ``mean``,
    ``m2`` (sum of squared deviations from the mean), ``min`` and ``max`` are
    [T, len(dc_names), len(metrics)].  The last entry of ``dc_names`` is the
    fleet row.  Cells with n == 0 hold NaN mean/min/max and m2 == 0."""
    time: np.ndarray
    n: np.ndarray
    mean: np.ndarray
    m2: np.ndarray
    min: np.ndarray
    max: np.ndarray
    metrics: List[str]
    dc_names: List[str]

    @classmethod
    def from_tensor(cls, stats, time, metrics, dc_names) -> "SeriesStats":
        """stats: [T, n_row, K, 5] = {n, mean, M2, min, max} (tensor or array,
        on the host), time: [T]."""
        a = np.asarray(stats, dtype=np.float64)
        return cls(time=np.asarray(time, dtype=np.float64).copy(),
                   n=a[..., 0].astype(np.int64), mean=a[..., 1].copy(),
                   m2=a[..., 2].copy(), min=a[..., 3].copy(),
                   max=a[..., 4].copy(), metrics=list(metrics),
                   dc_names=list(dc_names))

    def to_array(self) -> np.ndarray:
        """Inverse of from_tensor: [T, n_row, K, 5] float64."""
        return np.stack([self.n.astype(np.float64), self.mean, self.m2,
                         self.min, self.max], axis=-1)

    def trimmed(self) -> "SeriesStats":
        """Drop the ticks no replica has reached."""
        keep = self.n.reshape(len(self.time), -1).max(axis=1) > 0 \
            if self.n.size else np.zeros(len(self.time), bool)
        return SeriesStats(self.time[keep], self.n[keep], self.mean[keep],
                           self.m2[keep], self.min[keep], self.max[keep],
                           self.metrics, self.dc_names)


def _pad_ticks(s: SeriesStats, T: int) -> SeriesStats:
    """Extend to T ticks with empty cells (n = 0)."""
    extra = T - len(s.time)
    if extra <= 0:
        return s
    shape = (extra,) + s.n.shape[1:]
    nan = np.full(shape, np.nan)
    return SeriesStats(
        np.concatenate([s.time, np.full(extra, np.nan)]),
        np.concatenate([s.n, np.zeros(shape, np.int64)]),
        np.concatenate([s.mean, nan]), np.concatenate([s.m2, np.zeros(shape)]),
        np.concatenate([s.min, nan]), np.concatenate([s.max, nan]),
        s.metrics, s.dc_names)


def _merge_pair(a: SeriesStats, b: SeriesStats) -> SeriesStats:
    """Chan et al. parallel combination of (n, mean, M2) per cell; an empty
    side contributes nothing (its NaN mean never enters the arithmetic)."""
    assert a.metrics == b.metrics and a.dc_names == b.dc_names
    T = max(len(a.time), len(b.time))
    a, b = _pad_ticks(a, T), _pad_ticks(b, T)
    na, nb = a.n.astype(np.float64), b.n.astype(np.float64)
    n = na + nb
    ea, eb = a.n == 0, b.n == 0
    ma, mb = np.where(ea, 0.0, a.mean), np.where(eb, 0.0, b.mean)
    delta = mb - ma
    safe_n = np.where(n > 0, n, 1.0)
    mean = ma + delta * (nb / safe_n)
    m2 = a.m2 + b.m2 + delta * delta * (na * nb / safe_n)
    mean = np.where(ea, b.mean, np.where(eb, a.mean, mean))
    m2 = np.where(ea, b.m2, np.where(eb, a.m2, m2))
    # a tick's time comes from whichever side has reached it
    a_has = (a.n.reshape(T, -1).max(axis=1) > 0) if a.n.size \
        else np.zeros(T, bool)
    return SeriesStats(np.where(a_has, a.time, b.time), a.n + b.n, mean, m2,
                       np.fmin(a.min, b.min), np.fmax(a.max, b.max),
                       a.metrics, a.dc_names)


def merge_series_stats(parts: Sequence[SeriesStats]) -> SeriesStats:
    """Combine the statistics of disjoint replica groups (shards, ranks,
    separate runs) into those of their union: pairwise (tree-order) Chan
    merge of n / mean / M2, min and max merged directly."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_series_stats needs at least one SeriesStats")
    while len(parts) > 1:
        nxt = [_merge_pair(parts[i], parts[i + 1])
               for i in range(0, len(parts) - 1, 2)]
        if len(parts) % 2:
            nxt.append(parts[-1])
        parts = nxt
    return parts[0]


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
    multi = n > 1
    std = np.where(multi, np.sqrt(np.maximum(stats.m2.reshape(-1), 0.0)
                                  / np.where(multi, n - 1, 1)), 0.0)
    se = np.where(multi, std / np.sqrt(np.where(multi, n, 1)), 0.0)
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
