"""Host-side Philox4x32-10 and the distribution recipes of the device RNG
(ops/csrc/hip/philox.hpp), formula for formula in plain `math`.

Two users:
  * BatchedEngine._seed_arrivals draws the first arrival of every stream
    here; the kernel continues the same stream from ctr = n_streams.
  * the tests use it as the numerics reference for the device:
    tests/test_philox_cpu.py pins philox4x32 to the Random123 known-answer
    vectors and every recipe to mpmath; tests/test_gpu_rng.py compares the
    device words, draws and word -> value maps with it and replays whole
    replica streams against a finished BatchedEngine run.

A draw takes (key, ctr) and consumes exactly one counter, like its device
twin; the `*_map` functions are the word -> value halves."""
import math

from ..models.arrivals import profile_gap  # noqa: F401  (the twin itself)

M0 = 0xD2511F53
M1 = 0xCD9E8D57
B0 = 0x9E3779B9
B1 = 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32(key: int, ctr: int, c2: int = 0, c3: int = 0):
    """One Philox4x32-10 block.  `ctr` holds counter words 0 and 1 (the device
    only ever uses those); `c2`, `c3` are the upper two words."""
    c0 = ctr & MASK
    c1 = (ctr >> 32) & MASK
    c2 &= MASK
    c3 &= MASK
    k0 = key & MASK
    k1 = (key >> 32) & MASK
    for _ in range(10):
        p0 = (M0 * c0) & 0xFFFFFFFFFFFFFFFF
        p1 = (M1 * c2) & 0xFFFFFFFFFFFFFFFF
        h0, l0 = (p0 >> 32) & MASK, p0 & MASK
        h1, l1 = (p1 >> 32) & MASK, p1 & MASK
        c0, c1, c2, c3 = (h1 ^ c1 ^ k0) & MASK, l1, (h0 ^ c3 ^ k1) & MASK, l0
        k0 = (k0 + B0) & MASK
        k1 = (k1 + B1) & MASK
    return c0, c1, c2, c3


def u01_map(w0: int, w1: int) -> float:
    a, b = w0 >> 5, w1 >> 6
    return (a * 67108864.0 + b) * (1.0 / 9007199254740992.0)


def philox_u01(key: int, ctr: int) -> float:
    w = philox4x32(key, ctr)
    return u01_map(w[0], w[1])


def philox_u01_pair(key: int, ctr: int):
    w = philox4x32(key, ctr)
    return u01_map(w[0], w[1]), u01_map(w[2], w[3])


def rexp_map(u: float, lambd: float) -> float:
    return -math.log(1.0 - u) / lambd


def rexp(key: int, ctr: int, lambd: float) -> float:
    return rexp_map(philox_u01(key, ctr), lambd)


def rbelow_map(w0: int, n: int) -> int:
    return (w0 * n) >> 32


def rbelow(key: int, ctr: int, n: int) -> int:
    return rbelow_map(philox4x32(key, ctr)[0], n)


def rnormal_map(ua: float, ub: float, mu: float, sigma: float) -> float:
    r = math.sqrt(-2.0 * math.log(1.0 - ua))
    z = r * math.cos(2.0 * math.pi * ub)
    return mu + z * sigma


def rnormal(key: int, ctr: int, mu: float, sigma: float) -> float:
    return rnormal_map(*philox_u01_pair(key, ctr), mu, sigma)


def rlognormal_map(ua: float, ub: float, mu: float, sigma: float) -> float:
    return math.exp(rnormal_map(ua, ub, mu, sigma))


def rlognormal(key: int, ctr: int, mu: float, sigma: float) -> float:
    return rlognormal_map(*philox_u01_pair(key, ctr), mu, sigma)


def rpareto_inf_map(u01: float) -> float:
    u = max(1e-9, 1.0 - u01)
    return 1.0 / math.pow(u, 1.0 / 1.8)


def rpareto_inf(key: int, ctr: int) -> float:
    return rpareto_inf_map(philox_u01(key, ctr))


THIN_MAX_ITER = 4096
D_INF = 1e300   # the device's "never": a process that is off


def draw_interarrival(key: int, ctr: int, t: float, mode: str, rate: float,
                      amp: float = 0.0, period: float = 1.0, trace=None):
    """Inter-arrival after an arrival at time t -> (ia, counter afterwards):
    the device draw_interarrival.  Poisson takes one draw; sinusoid thinning
    takes two per iteration (candidate gap, then acceptance).  `trace`, if a
    list, receives (u, threshold) of every acceptance test."""
    ia = D_INF
    if mode == "poisson" and rate > 0:
        ia = rexp(key, ctr, rate)
        ctr += 1
    elif mode == "sinusoid":
        max_rate = rate * (1.0 + abs(amp))
        if max_rate > 0:
            for _ in range(THIN_MAX_ITER):
                w = rexp(key, ctr, max_rate)
                lam = max(0.0, rate * (1.0 + amp * math.sin(
                    2.0 * math.pi * math.fmod(t + w, period) / period)))
                u = philox_u01(key, ctr + 1)
                ctr += 2
                if trace is not None:
                    trace.append((u, lam / max_rate))
                if u <= lam / max_rate:
                    ia = w
                    break
    return ia, ctr


def draw_profile_gap(key: int, ctr: int, t: float, rate: float, period: float,
                     m, cum):
    """Profile-mode inter-arrival -> (ia, counter afterwards): one unit
    exponential at ``ctr``; an off stream draws nothing."""
    if not (rate > 0 and cum[len(m)] > 0):
        return D_INF, ctr
    E = rexp_map(philox_u01(key, ctr), 1.0)
    return profile_gap(E, t, rate, period, m, cum), ctr + 1


def replica_key(seed: int, global_replica_id: int) -> int:
    return (seed ^ ((0x9E3779B97F4A7C15 * global_replica_id) & 0xFFFFFFFFFFFFFFFF)) \
        & 0xFFFFFFFFFFFFFFFF
