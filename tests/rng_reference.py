"""Shared reference data for the RNG tests (test_philox_cpu.py on the host,
test_gpu_rng.py on the device): the rows of Philox words both files test, the
recipes of ops/csrc/hip/philox.hpp in mpmath at 120 bits, and the error
measure (ulps of the reference value).

The mpmath recipes are the formulas as the source writes them, on the same
f64 inputs and with the same f64 constants (M_PI, 1.0 / 1.8, the engine's
mu = log(50000) rounded to f64); only the arithmetic and the transcendental
calls are carried out at 120 bits.  So the measured error is the rounding of
the recipe's own operations, not of its constants."""
import functools
import math

import mpmath
import numpy as np

from distributed_cluster_gpus_amd.engine import _philox_host as ph

MP = mpmath.mp.clone()
MP.prec = 120

# the engine's parameters: training sizes are lognormal(log 50000, 0.4), the
# paper's sinusoid thinning draws its candidate gaps at rate 6 * (1 + 0.6)
MU = math.log(50000.0)
SIGMA = 0.4
LAMBD = 6.0 * (1.0 + abs(0.6))
N_BELOW = 8          # the paper scenario's DC count

W_MAX = 0xFFFFFFFF
U_MAX = 1.0 - 2.0 ** -53
PARETO_CAP = 1e-9    # rpareto_inf clamps 1 - u01 from below here

RECIPES = ("rexp", "rnormal", "rlognormal", "rpareto_inf")


def words_for_u(k: int):
    """(w0, w1) whose u01 is k * 2**-53."""
    assert 0 <= k < 2 ** 53
    return (k >> 26) << 5, (k & (2 ** 26 - 1)) << 6


def _edge_rows():
    """(name, (w0, w1, w2, w3), n_below)"""
    rows = [("zero", (0, 0, 0, 0), N_BELOW),
            ("ones", (W_MAX,) * 4, N_BELOW)]
    # Box-Muller corners: ua in {0, max} x ub in {0, 1/4, 1/2, max}
    ub_words = {"0": (0, 0), "1/4": words_for_u(2 ** 51),
                "1/2": words_for_u(2 ** 52), "max": (W_MAX, W_MAX)}
    for ua_name, wa in (("0", (0, 0)), ("max", (W_MAX, W_MAX))):
        for ub_name, wb in ub_words.items():
            rows.append((f"bm ua={ua_name} ub={ub_name}", wa + wb, N_BELOW))
    # the Pareto clamp: 1 - u01 = k * 2**-53 just below and just above 1e-9
    # (1e-9 * 2**53 = 9007199.25...), then far inside the clamp
    for k in (9007199, 9007200, 1):
        rows.append((f"pareto 1-u={k}*2^-53",
                     words_for_u(2 ** 53 - k) + (0x9E3779B9, 0x7F4A7C15),
                     N_BELOW))
    # rbelow at the top word
    for n in (1, 8, 2 ** 32 - 1):
        rows.append((f"rbelow n={n}", (W_MAX, 0x12345678, 0, 1), n))
    # the low bits the combiner must drop, and the lowest it must keep
    rows.append(("dropped bits", (0x1F, 0x3F, 0x1F, 0x3F), N_BELOW))
    rows.append(("lowest kept bits", (0x20, 0x40, 0x20, 0x40), N_BELOW))
    return rows


EDGE_ROWS = _edge_rows()
N_RANDOM = 480


@functools.lru_cache(maxsize=None)
def word_rows():
    """(words int64[B,4], n_below int64[B]): the edge rows, then random ones;
    B <= 512."""
    rng = np.random.default_rng(950)
    w = [r[1] for r in EDGE_ROWS]
    n = [r[2] for r in EDGE_ROWS]
    w += rng.integers(0, 2 ** 32, size=(N_RANDOM, 4)).tolist()
    n += [N_BELOW] * N_RANDOM
    words = np.asarray(w, dtype=np.int64)
    n_below = np.asarray(n, dtype=np.int64)
    assert words.shape[0] <= 512
    words.setflags(write=False)
    n_below.setflags(write=False)
    return words, n_below


def edge_index(name: str) -> int:
    return [r[0] for r in EDGE_ROWS].index(name)


# ------------------------------------------------------------ mpmath recipes

def mp_rexp(u, lambd=LAMBD):
    return -MP.log(1 - MP.mpf(u)) / MP.mpf(lambd)


def mp_rnormal(ua, ub, mu=MU, sigma=SIGMA):
    r = MP.sqrt(-2 * MP.log(1 - MP.mpf(ua)))
    z = r * MP.cos(2 * MP.mpf(math.pi) * MP.mpf(ub))
    return MP.mpf(mu) + z * MP.mpf(sigma)


def mp_rlognormal(ua, ub, mu=MU, sigma=SIGMA):
    return MP.exp(mp_rnormal(ua, ub, mu, sigma))


def mp_rpareto_inf(u01):
    u = max(MP.mpf(PARETO_CAP), 1 - MP.mpf(u01))
    return 1 / MP.power(u, MP.mpf(1.0 / 1.8))


def ulp_error(x: float, ref) -> float:
    """|x - ref| in ulps of ref (ref an mpf)."""
    return float(abs(MP.mpf(x) - ref) / MP.mpf(math.ulp(float(ref))))


@functools.lru_cache(maxsize=None)
def uniforms():
    """(ua, ub) per word row, by the host combiner (exact arithmetic)."""
    words, _ = word_rows()
    return [(ph.u01_map(int(w[0]), int(w[1])), ph.u01_map(int(w[2]), int(w[3])))
            for w in words]


@functools.lru_cache(maxsize=None)
def mp_reference():
    """recipe -> list of mpf, one per word row."""
    us = uniforms()
    return {"rexp": [mp_rexp(ua) for ua, _ in us],
            "rnormal": [mp_rnormal(ua, ub) for ua, ub in us],
            "rlognormal": [mp_rlognormal(ua, ub) for ua, ub in us],
            "rpareto_inf": [mp_rpareto_inf(ua) for ua, _ in us]}


@functools.lru_cache(maxsize=None)
def host_values():
    """recipe -> list of float by the plain host recipes (math, libm)."""
    us = uniforms()
    return {"rexp": [ph.rexp_map(ua, LAMBD) for ua, _ in us],
            "rnormal": [ph.rnormal_map(ua, ub, MU, SIGMA) for ua, ub in us],
            "rlognormal": [ph.rlognormal_map(ua, ub, MU, SIGMA)
                           for ua, ub in us],
            "rpareto_inf": [ph.rpareto_inf_map(ua) for ua, _ in us]}


def max_ulp_error(values, recipe: str) -> float:
    ref = mp_reference()[recipe]
    return max(ulp_error(float(x), r) for x, r in zip(values, ref))


# Largest error of the plain host recipes against mpmath over word_rows(), in
# ulps of the result, measured on the CPU (glibc 2.x libm) and rounded up to
# two decimals; test_philox_cpu.py asserts the host stays within it.  The
# device bound is twice that plus 2 ulp: the device library may round each of
# the up to two transcendental calls one ulp differently, and the
# amplification through exp is the same on both sides.
HOST_MAX_ULP = {"rexp": 1.24, "rnormal": 0.65, "rlognormal": 8.41,
                "rpareto_inf": 1.31}


def device_bound(recipe: str) -> float:
    return 2.0 * HOST_MAX_ULP[recipe] + 2.0


# ------------------------------------------------------- whole-stream replay
#
# For a non-RL algorithm the arrival process is open-loop: nothing the
# cluster does feeds back into the random stream.  Per arrival the kernel
# draws, in this order, the size (rpareto_inf for inference, max(0.1,
# rlognormal) for training), the DC (rbelow(n_dc); eco_route scores instead
# of drawing) and the inter-arrival (1 draw for Poisson, 2 per thinning
# iteration).  Streams (index = ingress * 2 + job type) are merged by time,
# lower stream index first; everything with t <= end_time is processed; the
# counter starts at n_streams, after the host's seed draws.

class Replay:
    """What one replica's random stream must have produced by end_time."""

    def __init__(self, n_streams):
        self.ctr = n_streams
        self.jid = 0
        self.arr_next = None
        self.n_arrivals = [0] * n_streams
        # jid -> (ingress, job type, dc or None, host size, mpmath size)
        self.jobs = {}
        self.min_gap = math.inf        # between consecutive merged arrivals
        self.min_margin = math.inf     # |u - threshold| over thinning tests


def replay_replica(seed, global_id, first_arrivals, arrivals, n_dc, end_time,
                   draws_dc=True):
    """`first_arrivals`: the stream's seed row (BatchedEngine._seed_arrivals);
    `arrivals`: (inference, training) ArrivalProcess."""
    key = ph.replica_key(seed, global_id)
    ns = len(first_arrivals)
    out = Replay(ns)
    nxt = [float(x) for x in first_arrivals]
    last_t = None
    while True:
        s = min(range(ns), key=lambda k: (nxt[k], k))
        t = nxt[s]
        if t > end_time:
            break
        if last_t is not None:
            out.min_gap = min(out.min_gap, t - last_t)
        last_t = t
        out.jid += 1
        out.n_arrivals[s] += 1
        jt = s & 1
        if jt == 0:
            u = ph.philox_u01(key, out.ctr)
            size = ph.rpareto_inf_map(u)
            size_mp = mp_rpareto_inf(u)
        else:
            ua, ub = ph.philox_u01_pair(key, out.ctr)
            size = max(0.1, ph.rlognormal_map(ua, ub, MU, SIGMA))
            size_mp = max(MP.mpf(0.1), mp_rlognormal(ua, ub))
        out.ctr += 1
        dc = None
        if draws_dc:
            dc = ph.rbelow(key, out.ctr, n_dc)
            out.ctr += 1
        out.jobs[out.jid] = (s >> 1, jt, dc, size, size_mp)
        arr = arrivals[jt]
        trace = []
        ia, out.ctr = ph.draw_interarrival(key, out.ctr, t, arr.mode, arr.rate,
                                           arr.amp, arr.period, trace)
        for u, thr in trace:
            out.min_margin = min(out.min_margin, abs(u - thr))
        nxt[s] = t + ia
    out.arr_next = nxt
    return out
