"""Shared reference data for the rate-profile tests (test_arrival_profile_cpu.py
on the host, test_gpu_arrival_profile.py on the device): the edge cases of the
inversion, the Fraction-exact integrated rate, and the paper-scenario tables
both files use."""
import functools
import math
from fractions import Fraction

import numpy as np

from distributed_cluster_gpus_amd.models.arrivals import (ArrivalProcess,
                                                          profile_tables)

# the issue's count / replay configuration
K5 = 5
PERIOD = 120.0
DURATION = 600.0
RATE_INF, RATE_TRN = 1.5, 0.25
BASE_INF = (0.0, 0.5, 2.0, 1.0, 1.5)
BASE_TRN = (1.0, 0.0, 0.0, 3.0, 1.0)
N_ING = 8


def rotations(base, n=N_ING):
    return np.array([np.roll(np.asarray(base, np.float64), i)
                     for i in range(n)])


def paper_profiles(period=PERIOD, zero_row=None):
    """(inference, training) in profile mode: row i is the base rotated by i;
    ``zero_row`` turns that ingress's inference stream off."""
    inf = rotations(BASE_INF)
    if zero_row is not None:
        inf[zero_row] = 0.0
    return (ArrivalProcess(mode="profile", rate=RATE_INF, period=period,
                           profile=inf),
            ArrivalProcess(mode="profile", rate=RATE_TRN, period=period,
                           profile=rotations(BASE_TRN)))


def exact_Lambda(t, g, rate, period, m):
    """integral_t^{t+g} rate * m[floor(K * frac(s / period))] ds, exactly."""
    K = len(m)
    mf = [Fraction(v) for v in m]
    M = sum(mf) / K

    def L(s):
        cyc = s / period
        n = math.floor(cyc)
        x = cyc - n
        k0 = min(K - 1, math.floor(x * K))
        return n * M + sum(mf[:k0]) / K + (x - Fraction(k0, K)) * mf[k0]

    t, g, period = Fraction(t), Fraction(g), Fraction(period)
    return Fraction(rate) * period * (L(t + g) - L(t))


def lambda_tolerance(t, g, rate, period, m):
    """16 roundings of at most one ulp of a time no larger than t + g +
    period, each worth rate * max(m) of integrated rate."""
    return 16.0 * rate * max(m) * math.ulp(t + g + period)


def _edge_rows():
    """(name, m, rate, period, t, E)"""
    k64 = [((7 * k) % 11) / 4.0 for k in range(64)]
    k64[0] = k64[63] = 0.0
    rows = [
        ("K=1", [2.5], 1.5, 120.0, 37.25, 0.8),
        ("K=1 three cycles", [1.0], 0.5, 10.0, 3.0, 16.0),
        ("K=5", list(BASE_INF), 1.5, 120.0, 31.7, 1.3),
        ("K=64", k64, 2.0, 300.0, 123.456, 2.2),
        ("K=64 late", k64, 2.0, 300.0, 299.99, 0.01),
        ("segment boundary", [1.0, 0.5, 2.0, 1.0, 1.5], 1.5, 120.0, 48.0, 0.4),
        ("segment boundary into zero", list(BASE_TRN), 0.25, 120.0, 24.0, 0.3),
        ("cycle boundary", list(BASE_INF), 1.5, 120.0, 240.0, 0.7),
        ("cycle boundary t=0", list(BASE_TRN), 0.25, 120.0, 0.0, 0.05),
        ("zero at start", [0.0, 0.0, 1.0, 2.0, 1.0], 1.0, 100.0, 5.0, 0.5),
        ("zero in the middle", [1.0, 0.0, 0.0, 3.0, 1.0], 1.0, 100.0, 19.0, 0.9),
        ("zero at the end", [1.0, 2.0, 1.0, 0.0, 0.0], 1.0, 100.0, 59.0, 0.5),
        ("starts inside a zero run", [1.0, 2.0, 1.0, 0.0, 0.0], 1.0, 100.0,
         75.0, 0.01),
        # rate * period * M = 1.5 * 120 * 1 = 180 per cycle
        ("E spans three cycles", list(BASE_INF), 1.5, 120.0, 100.0, 3.2 * 180.0),
        ("E=0", list(BASE_INF), 1.5, 120.0, 31.7, 0.0),
        ("E=0 on a boundary before zeros", list(BASE_TRN), 0.25, 120.0, 24.0,
         0.0),
        ("E tiny", list(BASE_INF), 1.5, 120.0, 77.0, 2.0 ** -60),
        ("late t", list(BASE_INF), 1.5, 120.0, 86400.0 * 7 + 13.0, 1.1),
    ]
    return rows


EDGE_ROWS = _edge_rows()
OFF_ROWS = [("rate=0", list(BASE_INF), 0.0, 120.0, 3.0, 1.0),
            ("all-zero row", [0.0] * 5, 1.5, 120.0, 3.0, 1.0)]


@functools.lru_cache(maxsize=None)
def random_rows(n=3000, seed=355):
    """n random (m, rate, period, t, E) rows: K over 1..64, zeros sprinkled
    in, t over many cycles, E from tiny to several cycles."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        K = int(rng.choice([1, 2, 3, 5, 8, 9, 24, 63, 64]))
        m = rng.uniform(0.0, 3.0, K)
        m[rng.random(K) < 0.25] = 0.0
        if not m.any():
            m[int(rng.integers(K))] = 1.0
        period = float(rng.choice([1.0, 120.0, 300.0, 86400.0, 97.3]))
        rate = float(rng.choice([0.25, 1.5, 6.0, 40.0]))
        t = float(rng.uniform(0.0, 12.0) * period)
        E = float(rng.exponential(1.0) * rng.choice([1e-6, 1.0, 1.0, 50.0]))
        out.append((m.tolist(), rate, period, t, E))
    return out


def tables(m):
    return profile_tables(m)
