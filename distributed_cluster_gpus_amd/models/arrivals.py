"""Arrival processes and job-size distributions.

Capability parity: reference simcore/arrivals.py.  Two deliberate behavioural
notes, both preserved for log parity (SURVEY.md §6 reproduction note /
Appendix A.1):

* Sinusoid arrivals use thinning whose rejection loop re-derives the candidate
  time from the SAME base ``t`` each iteration (it does not accumulate rejected
  gaps), which biases the effective rate toward rate*(1+|amp|).  The faithful
  form is the default; ``accumulate=True`` gives the textbook-correct thinning.
* Inference sizes are Pareto(x_m=1, alpha=1.8); training sizes are
  lognormal(mu=ln 50000, sigma=0.4) floored at 0.1.

RNG is dependency-injected (any object with the ``random.Random`` API) so the
scalar engines can share one CPython-compatible Mersenne stream.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

PROFILE_MAX_SEGMENTS = 64
D_INF = 1e300   # the batched engine's "never" (engine/_philox_host.py)

# job-size distribution constants (reference: simcore/arrivals.py:5-11)
PARETO_XM = 1.0
PARETO_ALPHA = 1.8
LOGNORM_MU = math.log(50000.0)
LOGNORM_SIGMA = 0.4
TRAIN_SIZE_FLOOR = 0.1


def sample_job_size(jtype: str, rng) -> float:
    """Draw a job size in abstract work units for 'inference' or 'training'."""
    if jtype == "inference":
        u = max(1e-9, 1.0 - rng.random())
        return PARETO_XM / (u ** (1.0 / PARETO_ALPHA))
    return max(TRAIN_SIZE_FLOOR, rng.lognormvariate(LOGNORM_MU, LOGNORM_SIGMA))


def _expovariate_safe(rng, lmbda: float) -> float:
    return float("inf") if lmbda <= 0 else rng.expovariate(lmbda)


@dataclass
class ArrivalProcess:
    """Inter-arrival generator: 'poisson' | 'sinusoid' | 'off' | 'profile'.

    'profile' is a piecewise-constant rate per ingress: ``profile`` holds K
    multipliers (shape [K], shared by every ingress, or [n_ing, K]), ``rate``
    scales them and ``period`` is the cycle, so ingress i runs at
    ``rate * m_i[floor(K * frac(t / period))]``.  A row of zeros turns that
    ingress off; ``amp`` is unused.  Gaps are drawn by exact inversion
    (``profile_gap``), one unit exponential per arrival."""
    mode: str
    rate: float
    amp: float = 0.0
    period: float = 3600.0
    accumulate: bool = False  # True = textbook thinning (documented divergence)
    profile: Optional[np.ndarray] = None

    def __post_init__(self):
        if self.mode == "profile":
            self.profile = check_profile(self.profile)
            if not (math.isfinite(self.period) and self.period > 0):
                raise ValueError(f"profile period = {self.period} must be > 0")
            self._tables = [profile_tables(row) for row in self.profile]

    # ---------------- profile mode ----------------
    def profile_rows(self, n_ing: int) -> np.ndarray:
        """The [n_ing, K] multiplier table (a single row is shared)."""
        rows = self.profile.shape[0]
        if rows not in (1, int(n_ing)):
            raise ValueError(
                f"profile has {rows} rows; it needs 1 (shared) or n_ing = "
                f"{n_ing}")
        return np.broadcast_to(self.profile, (int(n_ing), self.profile.shape[1]))

    def _table(self, ingress: int):
        if len(self._tables) == 1:
            return self._tables[0]
        if not 0 <= int(ingress) < len(self._tables):
            raise ValueError(f"ingress {ingress} outside the profile's "
                             f"{len(self._tables)} rows")
        return self._tables[int(ingress)]

    @classmethod
    def diurnal(cls, rate, amp, period, offsets_s, segments=24):
        """Profile-mode twin of a sinusoid, shifted per ingress: ingress i
        follows ``1 + amp * sin(2 pi (t - offsets_s[i]) / period)`` (clamped at
        0), each of the ``segments`` multipliers being that segment's mean, so
        an unclamped row averages 1."""
        K = int(segments)
        if not 1 <= K <= PROFILE_MAX_SEGMENTS:
            raise ValueError(f"segments = {segments} outside [1, "
                             f"{PROFILE_MAX_SEGMENTS}]")
        offs = np.atleast_1d(np.asarray(offsets_s, dtype=np.float64))
        k = np.arange(K, dtype=np.float64)
        # mean of sin(2 pi (x - o)) over [k/K, (k+1)/K]
        o = (offs / float(period))[:, None]
        a = 2.0 * np.pi * (k / K - o)
        b = 2.0 * np.pi * ((k + 1.0) / K - o)
        mean_sin = (np.cos(a) - np.cos(b)) * (K / (2.0 * np.pi))
        tab = np.maximum(0.0, 1.0 + float(amp) * mean_sin)
        return cls(mode="profile", rate=float(rate), amp=float(amp),
                   period=float(period), profile=tab)

    @classmethod
    def from_csv(cls, path, rate, period, amp=0.0):
        """Profile mode from a CSV of n_ing rows x K columns of multipliers
        (one row: shared by every ingress)."""
        return cls(mode="profile", rate=float(rate), amp=float(amp),
                   period=float(period), profile=load_profile_csv(path))

    def lambda_t(self, t: float, ingress: int = 0) -> float:
        if self.mode == "profile":
            m, _ = self._table(ingress)
            K = len(m)
            x = math.fmod(t, self.period) / self.period
            return self.rate * m[min(K - 1, int(x * K))]
        if self.mode == "poisson":
            return self.rate
        if self.mode == "sinusoid":
            return max(0.0, self.rate * (1.0 + self.amp *
                                         math.sin(2.0 * math.pi * (t % self.period) / self.period)))
        if self.mode == "off":
            return 0.0
        raise ValueError(f"Unknown arrival mode {self.mode!r}")

    def next_interarrival(self, t: float, rng, ingress: int = 0) -> float:
        if self.mode == "profile":
            m, cum = self._table(ingress)
            if not (self.rate > 0 and cum[-1] > 0):
                return float("inf")       # off: no draw is consumed
            g = profile_gap(rng.expovariate(1.0), t, self.rate, self.period,
                            m, cum)
            return float("inf") if g >= D_INF else g
        if self.mode == "poisson":
            return _expovariate_safe(rng, self.rate)
        if self.mode == "sinusoid":
            max_rate = self.rate * (1.0 + abs(self.amp))
            elapsed = 0.0
            while True:
                w = _expovariate_safe(rng, max_rate)
                if self.accumulate:
                    elapsed += w
                    if rng.random() <= self.lambda_t(t + elapsed) / max_rate:
                        return elapsed
                else:
                    # faithful non-accumulating rejection (reference arrivals.py:39-44)
                    if rng.random() <= self.lambda_t(t + w) / max_rate:
                        return w
        if self.mode == "off":
            return float("inf")
        raise ValueError(f"Unknown arrival mode {self.mode!r}")


def profile_gap(E: float, t: float, rate: float, period: float, m, cum):
    """Gap g >= 0 after an arrival at t with integral_t^{t+g} lambda = E, for
    the piecewise-constant rate ``rate * m[floor(K * frac(t / period))]``:
    exact inversion, the host twin of the device profile_gap
    (ops/csrc/hip/arrival_ring.hpp) and of the native core's, IEEE operation
    for operation.  ``cum[k] =
    (m[0] + ... + m[k-1]) / K`` (K + 1 entries).  D_INF where the stream is
    off; the caller then consumes no draw."""
    K = len(m)
    M = cum[K]
    if not (rate > 0 and M > 0):
        return D_INF
    x = math.fmod(t, period) / period
    k0 = min(K - 1, int(x * K))
    A = cum[k0] + (x - k0 / K) * m[k0]
    T = A + E / (rate * period)
    n = math.floor(T / M)
    Tp = T - n * M
    if Tp >= M:
        Tp -= M
        n += 1
    if Tp < 0:
        Tp = 0.0
    k = K - 1
    for j in range(K):
        if cum[j + 1] > Tp:
            k = j
            break
    xp = k / K + (Tp - cum[k]) / m[k]
    return max(0.0, (n + xp - x) * period)


def check_profile(profile) -> np.ndarray:
    """A profile as a read-only f64 [rows, K] array; ValueError, naming the
    offending value, for anything that is not one."""
    if profile is None:
        raise ValueError("mode 'profile' needs profile= (K multipliers, or "
                         "[n_ing, K])")
    try:
        p = np.array(profile, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"profile is not a numeric array: {profile!r}")
    if p.ndim == 1:
        p = p[None, :]
    if p.ndim != 2 or p.shape[0] < 1:
        raise ValueError(f"profile has shape {p.shape}; it needs [K] or "
                         "[n_ing, K]")
    K = p.shape[1]
    if not 1 <= K <= PROFILE_MAX_SEGMENTS:
        raise ValueError(f"profile has K = {K} segments; K must lie in [1, "
                         f"{PROFILE_MAX_SEGMENTS}]")
    bad = ~np.isfinite(p)
    if bad.any():
        i, k = np.argwhere(bad)[0]
        raise ValueError(f"profile[{i}, {k}] = {p[i, k]} is not finite")
    if (p < 0).any():
        i, k = np.argwhere(p < 0)[0]
        raise ValueError(f"profile[{i}, {k}] = {p[i, k]} is negative; a "
                         "multiplier must be >= 0")
    p.setflags(write=False)
    return p


def profile_tables(row):
    """``(m, cum)`` of one profile row as tuples of floats: ``cum[k] = (m[0] +
    ... + m[k-1]) / K``, summed left to right, K + 1 entries."""
    m = tuple(float(v) for v in row)
    K = len(m)
    cum, acc = [0.0], 0.0
    for v in m:
        acc += v
        cum.append(acc / K)
    return m, tuple(cum)


def load_profile_csv(path) -> np.ndarray:
    """n_ing rows x K columns of multipliers; '#' lines are comments."""
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            try:
                rows.append([float(x) for x in line.split(",") if x.strip()])
            except ValueError:
                raise ValueError(f"{path}:{ln}: not a row of numbers: {line!r}")
    if not rows or len({len(r) for r in rows}) != 1:
        raise ValueError(f"{path}: needs n_ing rows of the same K columns, "
                         f"found row lengths {[len(r) for r in rows]}")
    return check_profile(rows)
