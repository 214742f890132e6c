"""GPU tests for the analytic models and the (n, f) searches of
ops/csrc/hip/sim_models.hpp, through debug entry points that run the
production device templates (one 64-thread block per row; in the 8-lane build
every subgroup solves the same row), in both extensions.

  * d_job_power / d_unit_time against mpmath: relative error at most the
    expression's rounding depth x 2^-53 (P: c0*f, *f, *f, two sums, *n = 6;
    T: c1/f, two sums, /n = 4; all terms positive, so nothing amplifies).
  * the same against the unfused numpy f64 evaluation in source order.  The
    extension is compiled with floating-point contraction on, so the device
    fuses c0*f*f*f + c1*f + c2 and c2*n into FMAs and may differ from the
    unfused value in the last place.  The number of rows that differ bitwise
    is printed, not asserted; what is asserted is the bound both evaluations
    share through the exact value, twice the depth x 2^-53.
  * wave_grid_argmin / wave_energy_freq against a brute-force f64 scan
    (n-major, frequency-minor, first minimum), cross-checked against
    policies.gridsearch.best_nf_grid where their arithmetic coincides.
    Exact-arithmetic tables (small integers, power-of-two frequencies: every
    operation is exact, fused or not) pin the tie-break; random tables pin
    the pick up to the rounding of the score.

Score tolerances.  An f64 score is at most 12 roundings deep (6 for P, 4 for
T, the product, the objective factor), fused or not, so the device's and the
scan's value of one candidate differ by < 2 x 12 x 2^-53 relative; a pick is
therefore accepted when its reference score is <= min x (1 + 4 x 2^-52), and
must equal the scan's whenever the runner-up is further than that.  For the
fp32 ranking: at most 16 fp32 roundings per score, coefficient narrowing
included, 2^-24 each, on both candidates: <= min x (1 + 2^-18).
"""
import functools

import mpmath
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def gpu(fn):
    """the device tests; the checks of the tables themselves run anywhere"""
    return pytest.mark.gpu(pytest.mark.skipif(
        not torch.cuda.is_available(), reason="needs MI355X")(fn))


BUILDS = ("_sim_hip", "_sim_hip_mw")
EPS = 2.0 ** -53
TOL64 = 4 * 2.0 ** -52
TOL32 = 2.0 ** -18
J_PER_KWH = 3.6e6
# n_freq x n_max: the paper grid; idle lanes; a single candidate; two strided
# shapes (2 candidates per lane in the 64-lane build)
SHAPES = ((8, 8), (5, 3), (1, 1), (9, 8), (16, 8))


def _mod(name):
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    return load_sim_hip(name)


def _cu(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.copy()).cuda()


# ------------------------------------------------------------ host references

def np_gpu_power(f, pc):
    """unfused f64, in the source's order"""
    f = np.maximum(0.0, f)
    return ((pc[..., 0] * f) * f) * f + pc[..., 1] * f + pc[..., 2]


def np_job_power(n, f, pc):
    return np.maximum(0, n).astype(np.float64) * np_gpu_power(f, pc)


def np_unit_time(n, f, lc):
    n = np.maximum(1, n)
    f = np.maximum(1e-9, f)
    one = lc[..., 0] + lc[..., 1] / f
    many = (lc[..., 0] + lc[..., 1] / f + lc[..., 2] * n) / n
    return np.where(n == 1, one, many)


def np_scores(pc, lc, freq, n_max, objective, ci, price, ddl=None):
    """-> (score[B, n_cand] with +inf where the deadline rules a candidate
    out, n[n_cand], f[n_cand], T, P, E [B, n_cand]), candidates n-major"""
    n_freq = len(freq)
    cand = np.arange(n_max * n_freq)
    n = cand // n_freq + 1
    f = np.asarray(freq, dtype=np.float64)[cand % n_freq]
    pcb, lcb = pc[:, None, :], lc[:, None, :]
    T = np_unit_time(n[None, :], f[None, :], lcb)
    P = np_job_power(n[None, :], f[None, :], pcb)
    E = P * T
    if objective == 1:
        sc = E * ci[:, None]
    elif objective == 2:
        sc = (E / J_PER_KWH) * price[:, None]
    else:
        sc = E.copy()
    if ddl is not None:
        sc = np.where(T > ddl[:, None], np.inf, sc)
    return sc, n, f, T, P, E


MP = mpmath.mp.clone()
MP.prec = 120


def mp_models(pc, lc, n, f):
    m = MP.mpf
    fp = max(m(0), m(f))
    P = max(0, n) * (m(pc[0]) * fp ** 3 + m(pc[1]) * fp + m(pc[2]))
    nn = max(1, n)
    ft = max(m(1e-9), m(f))
    if nn == 1:
        T = m(lc[0]) + m(lc[1]) / ft
    else:
        T = (m(lc[0]) + m(lc[1]) / ft + m(lc[2]) * nn) / nn
    return P, T


def _rel(x, ref):
    if ref == 0:
        return 0.0 if x == 0 else float("inf")
    return float(abs(MP.mpf(float(x)) - ref) / abs(ref))


# ------------------------------------------------------------------ tables

def random_coeffs(rng, B):
    """positive coefficients in the paper's ranges"""
    pc = np.stack([rng.uniform(40, 105, B), rng.uniform(12, 90, B),
                   rng.uniform(35, 125, B)], axis=1)
    lc = np.stack([rng.uniform(0.004, 0.009, B), rng.uniform(0.0016, 0.06, B),
                   rng.uniform(0.0006, 0.0023, B)], axis=1)
    return pc, lc


def paper_coeffs():
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    sc = paper_scenario()
    return (np.asarray(sc.power_coeffs, dtype=np.float64).reshape(-1, 3),
            np.asarray(sc.latency_coeffs, dtype=np.float64).reshape(-1, 3),
            np.asarray(sc.freq_levels, dtype=np.float64))


def ladder(n_freq):
    if n_freq == 1:
        return np.array([0.7])
    return np.linspace(0.3, 1.0, n_freq)


@functools.lru_cache(maxsize=None)
def model_rows():
    """(pc, lc, n, f): edges, the paper's 16 triples over the ladder, random
    rows; 512 in all."""
    rng = np.random.default_rng(11)
    ppc, plc, pfreq = paper_coeffs()
    pc, lc, n, f = [], [], [], []
    for nn, ff in ((0, 0.7), (-3, 0.7), (1, 0.7), (1, 1e-9), (4, 1e-9),
                   (4, 0.0), (4, -1.0), (1, -0.5), (2, 1.0), (8, 0.3),
                   (0, 0.0), (1, 1e-10)):
        pc.append(ppc[3]); lc.append(plc[3]); n.append(nn); f.append(ff)
    n_edge = len(n)
    for t in range(16):
        for nn in (1, 3, 8):
            for ff in pfreq:
                pc.append(ppc[t]); lc.append(plc[t]); n.append(nn); f.append(ff)
    n_paper = len(n) - n_edge
    B = 512 - len(n)
    rpc, rlc = random_coeffs(rng, B)
    pc += list(rpc); lc += list(rlc)
    n += rng.integers(1, 9, B).tolist()
    f += rng.uniform(0.3, 1.0, B).tolist()
    out = (np.asarray(pc), np.asarray(lc), np.asarray(n, dtype=np.int32),
           np.asarray(f, dtype=np.float64))
    for a in out:
        a.setflags(write=False)
    return out + (n_edge, n_paper)


# ------------------------------------------------------------------ models

@gpu
@pytest.mark.parametrize("build", BUILDS)
def test_models_against_mpmath(build):
    pc, lc, n, f, n_edge, _ = model_rows()
    P, T = _mod(build).models_debug(_cu(pc), _cu(lc), _cu(n), _cu(f))
    P, T = P.cpu().numpy(), T.cpu().numpy()
    worst_p = worst_t = 0.0
    for i in range(len(n)):
        Pm, Tm = mp_models(pc[i], lc[i], int(n[i]), float(f[i]))
        worst_p = max(worst_p, _rel(P[i], Pm))
        worst_t = max(worst_t, _rel(T[i], Tm))
    print(f"{build}: P max rel error {worst_p / EPS:.3f} x 2^-53 (bound 6), "
          f"T {worst_t / EPS:.3f} x 2^-53 (bound 4)")
    assert worst_p <= 6 * EPS
    assert worst_t <= 4 * EPS
    # the edges, exactly: n <= 0 draws no power and takes one GPU's time,
    # f <= 0 leaves the constant term and the 1e-9 floor
    assert P[0] == 0.0 and P[1] == 0.0 and P[10] == 0.0
    assert T[0] == T[2] and T[1] == T[2]
    assert P[5] == 4 * pc[5, 2] and P[6] == 4 * pc[6, 2] and P[7] == pc[7, 2]
    assert T[5] == T[4] and T[6] == T[4] and T[7] == T[3] and T[11] == T[3]
    assert n_edge == 12


@gpu
@pytest.mark.parametrize("build", BUILDS)
def test_models_against_unfused_f64(build):
    pc, lc, n, f, n_edge, n_paper = model_rows()
    P, T = _mod(build).models_debug(_cu(pc), _cu(lc), _cu(n), _cu(f))
    P, T = P.cpu().numpy(), T.cpu().numpy()
    Ph, Th = np_job_power(n, f, pc), np_unit_time(n, f, lc)
    dp, dt = P != Ph, T != Th
    paper = slice(n_edge, n_edge + n_paper)
    rnd = slice(n_edge + n_paper, None)
    with np.errstate(invalid="ignore", divide="ignore"):
        up = np.nanmax(np.abs(P - Ph) / np.spacing(np.abs(Ph)))
        ut = np.nanmax(np.abs(T - Th) / np.spacing(np.abs(Th)))
    print(f"{build}: rows differing bitwise from the unfused evaluation: "
          f"P {int(dp[paper].sum())}/{n_paper} paper, "
          f"{int(dp[rnd].sum())}/{int(dp[rnd].size)} random; "
          f"T {int(dt[paper].sum())}/{n_paper} paper, "
          f"{int(dt[rnd].sum())}/{int(dt[rnd].size)} random; "
          f"largest difference P {up:.0f} ulp, T {ut:.0f} ulp")
    # both are within depth x 2^-53 of the exact value
    assert np.all(np.abs(P - Ph) <= 12 * EPS * np.abs(Ph))
    assert np.all(np.abs(T - Th) <= 8 * EPS * np.abs(Th))


# ------------------------------------------------------ exact tie-break tables

D = 1680.0      # divisible by every n <= 8 (and by 2): T = A / n stays exact
Q = 8.0


def tie_table(n_freq, n1, k1, n2, k2):
    """Integer coefficients and power-of-two frequencies such that, with the
    deadline D, candidate (n1, k1) is the first feasible minimum and (n2, k2)
    ties with it exactly (n1 <= n2).  Energy is p(f) * A(f) whatever n is,
    T = A(f) / n; frequency 1 sits at k1, 1/2 at k2, 1/4 everywhere else.

        A(1) = D n1, A(1/2) = D n2      -> first feasible at n1 resp. n2,
                                           with T == deadline exactly there
        p(1) = Q n2, p(1/2) = Q n1      -> both score Q D n1 n2
        p(1/4) = Q (3 n1 - n2) / 2 + 21 t, t large: far above the tie
    """
    assert n1 <= n2
    if k1 == k2:
        n2 = n1 + 1             # one frequency class: the tie is across n
    t = 64.0 * Q
    a, b = D * (2 * n1 - n2), D * (n2 - n1)
    alpha = 64.0 * t
    beta = 2 * Q * (n2 - n1) - 112.0 * t
    gamma = Q * n2 - alpha - beta
    freq = np.full(n_freq, 0.25)
    freq[k2] = 0.5
    freq[k1] = 1.0
    return (np.array([alpha, beta, gamma]), np.array([a, b, 0.0]), freq, D)


def _cand(n_freq, c):
    return c // n_freq + 1, c % n_freq


def exact_cases():
    """(name, n_freq, n_max, pc, lc, freq, has_ddl, ddl, expected candidate or
    None when nothing is feasible)"""
    cases = []
    for n_freq, n_max in SHAPES:
        fr = 2.0 ** -np.arange(n_freq)[::-1]        # ascending, ends at 1
        last = n_freq * n_max - 1
        # every candidate ties: E = n * 5 * (1680 / n)
        cases.append((f"all tie {n_freq}x{n_max}", n_freq, n_max,
                      np.array([0.0, 0.0, 5.0]), np.array([D, 0.0, 0.0]),
                      fr, False, 0.0, 0))
        # deadlines on T = (D + D / f) / n, smallest at the last candidate
        pc, lc = np.array([0.0, 0.0, 5.0]), np.array([D, D, 0.0])
        t_last = (D + D / fr[-1]) / n_max
        cases.append((f"none feasible {n_freq}x{n_max}", n_freq, n_max, pc,
                      lc, fr, True, t_last / 2, None))
        cases.append((f"only the last, T == ddl {n_freq}x{n_max}", n_freq,
                      n_max, pc, lc, fr, True, t_last, last))
        pairs = [(0, last)]
        if n_freq * n_max >= 64:
            pairs += [(15, 16), (31, 32), (0, 63)]
        if n_freq * n_max > 70:
            pairs += [(3, 67), (5, 70)]
        for i, j in pairs:
            if i == j:
                continue
            (n1, k1), (n2, k2) = _cand(n_freq, i), _cand(n_freq, j)
            pc, lc, freq, ddl = tie_table(n_freq, n1, k1, n2, k2)
            cases.append((f"tie {i}/{j} {n_freq}x{n_max}", n_freq, n_max, pc,
                          lc, freq, True, ddl, i))
    return cases


EXACT = exact_cases()


def _check_exact_case_on_host(case):
    """The construction itself, on the CPU: the scan picks the intended
    candidate, and the named partner ties with it exactly."""
    name, n_freq, n_max, pc, lc, freq, has_ddl, ddl, want = case
    sc, n, f, T, P, E = np_scores(pc[None], lc[None], freq, n_max, 0,
                                  np.ones(1), np.ones(1),
                                  np.array([ddl]) if has_ddl else None)
    sc = sc[0]
    if want is None:
        assert not np.isfinite(sc).any(), name
        return
    assert int(np.argmin(sc)) == want, name
    if name.startswith("tie "):
        j = int(name.split()[1].split("/")[1])
        assert sc[j] == sc[want], name
        assert np.sum(sc == sc[want]) >= 2
    if name.startswith("all tie"):
        assert np.all(sc == sc[0]), name
    if name.startswith("only the last"):
        assert np.isfinite(sc).sum() == 1 and T[0, want] == ddl, name
    # every feasible candidate's values are integers: exact in any evaluation
    ok = np.isfinite(sc)
    assert np.all(E[0][ok] == np.round(E[0][ok])), name


def test_exact_tables_are_what_they_claim():
    assert len(EXACT) > 30
    for case in EXACT:
        _check_exact_case_on_host(case)


@gpu
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("objective", (0, 1, 2))
def test_grid_tie_break_and_deadline_exact(build, objective):
    """Objectives 1 and 2 scale the energy by a positive factor, which keeps
    exact ties exact (equal operands, equal results) and the order."""
    m = _mod(build)
    for case in EXACT:
        name, n_freq, n_max, pc, lc, freq, has_ddl, ddl, want = case
        one = lambda v: _cu(np.array([v], dtype=np.float64))
        found, n, f, T, P, E = m.grid_argmin_debug(
            _cu(pc[None]), _cu(lc[None]), _cu(freq), n_max, objective,
            one(4.0), one(2.0), has_ddl, one(ddl), False)
        got = (int(found.item()), int(n.item()), f.item(), T.item(), P.item(),
               E.item())
        if want is None:
            assert got == (0, 1, 0.0, 0.0, 0.0, 0.0), name
            continue
        sc, ns, fs, Ts, Ps, Es = np_scores(pc[None], lc[None], freq, n_max, 0,
                                           np.ones(1), np.ones(1), None)
        assert got == (1, int(ns[want]), fs[want], Ts[0, want], Ps[0, want],
                       Es[0, want]), name


# ------------------------------------------------------------ random tables

@functools.lru_cache(maxsize=None)
def random_grid(n_freq, n_max, objective):
    """512 random positive tables and their scan: (pc, lc, freq, ci, price,
    scores[B, n_cand], n[n_cand], f[n_cand])"""
    rng = np.random.default_rng(1000 * n_freq + 10 * n_max + objective)
    B = 512
    pc, lc = random_coeffs(rng, B)
    ci = rng.uniform(50.0, 800.0, B)
    price = rng.uniform(0.03, 0.3, B)
    freq = ladder(n_freq)
    sc, n, f, *_ = np_scores(pc, lc, freq, n_max, objective, ci, price)
    for a in (pc, lc, ci, price, freq, sc):
        a.setflags(write=False)
    return pc, lc, freq, ci, price, sc, n, f


def _check_picks(sc, pick, tol, name):
    """pick[B]: candidate index the device chose"""
    B = sc.shape[0]
    rows = np.arange(B)
    best = sc.min(axis=1)
    first = sc.argmin(axis=1)
    assert np.all(sc[rows, pick] <= best * (1 + tol)), name
    if sc.shape[1] == 1:
        assert np.all(pick == 0)
        return 0.0
    runner = np.partition(sc, 1, axis=1)[:, 1]
    decided = runner > best * (1 + tol)
    assert np.all(pick[decided] == first[decided]), name
    return 1.0 - decided.mean()


@pytest.mark.parametrize("n_freq,n_max", SHAPES)
def test_random_tables_decide_on_the_cpu(n_freq, n_max):
    """The generator leaves under 1 % of rows to the tolerance (f64)."""
    for objective in (0, 1, 2):
        sc = random_grid(n_freq, n_max, objective)[5]
        if sc.shape[1] == 1:
            continue
        best = sc.min(axis=1)
        runner = np.partition(sc, 1, axis=1)[:, 1]
        assert np.mean(runner <= best * (1 + TOL64)) < 0.01


def test_scan_agrees_with_best_nf_grid():
    """The oracle's scan evaluates f ** 3 where the device source writes
    f * f * f, so scores can differ in the last place; picks must agree
    wherever the scan's runner-up is clear of that."""
    from distributed_cluster_gpus_amd.models.coeffs import (LatencyCoeffs,
                                                            PowerCoeffs)
    from distributed_cluster_gpus_amd.policies.gridsearch import best_nf_grid
    names = {0: "energy", 1: "carbon", 2: "cost"}
    for objective in (0, 1, 2):
        pc, lc, freq, ci, price, sc, n, f = random_grid(8, 8, objective)
        best = sc.min(axis=1)
        runner = np.partition(sc, 1, axis=1)[:, 1]
        for b in range(64):
            if runner[b] <= best[b] * (1 + TOL64):
                continue
            nb, fb, *_ = best_nf_grid(8, list(freq), PowerCoeffs(*pc[b]),
                                      LatencyCoeffs(*lc[b]), names[objective],
                                      ci[b], price[b])
            k = int(sc[b].argmin())
            assert (nb, fb) == (int(n[k]), float(f[k]))


def _pick_index(n, f, n_freq, freq):
    k = np.array([int(np.flatnonzero(freq == x)[0]) for x in f])
    return (n.astype(np.int64) - 1) * n_freq + k


@gpu
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fp32", (False, True))
@pytest.mark.parametrize("n_freq,n_max", SHAPES)
def test_grid_argmin_random(build, fp32, n_freq, n_max):
    m = _mod(build)
    for objective in (0, 1, 2):
        pc, lc, freq, ci, price, sc, ns, fs = random_grid(n_freq, n_max,
                                                          objective)
        B = len(ci)
        zero = torch.zeros(B, dtype=torch.float64, device="cuda")
        found, n, f, T, P, E = m.grid_argmin_debug(
            _cu(pc), _cu(lc), _cu(freq), n_max, objective, _cu(ci),
            _cu(price), False, zero, fp32)
        assert bool(found.all())
        n_h, f_h = n.cpu().numpy(), f.cpu().numpy()
        assert np.all((n_h >= 1) & (n_h <= n_max)) and np.isin(f_h, freq).all()
        pick = _pick_index(n_h, f_h, n_freq, freq)
        name = f"{build} fp32={fp32} {n_freq}x{n_max} obj={objective}"
        exempt = _check_picks(sc, pick, TOL32 if fp32 else TOL64, name)
        if not fp32:
            assert exempt < 0.01
        # T, P, E are the f64 models of the chosen candidate
        Pm, Tm = m.models_debug(_cu(pc), _cu(lc), n, f)
        assert torch.equal(T, Tm) and torch.equal(P, Pm), name
        assert torch.equal(E, Pm * Tm), name


@gpu
@pytest.mark.parametrize("build", BUILDS)
def test_grid_deadline_random(build):
    """A deadline at the median T of each row: the pick is feasible and the
    best feasible one.  Candidates whose T is within rounding of the deadline
    are left to either side."""
    m = _mod(build)
    for (n_freq, n_max), fp32 in (((8, 8), False), ((9, 8), False),
                                  ((8, 8), True)):
        pc, lc, freq, ci, price, _, ns, fs = random_grid(n_freq, n_max, 0)
        sc, _, _, T, _, _ = np_scores(pc, lc, freq, n_max, 0, ci, price)
        ddl = np.median(T, axis=1)
        tol_t = 2.0 ** -20 if fp32 else 8 * EPS
        sure_in = np.where(T <= ddl[:, None] * (1 - tol_t), sc, np.inf)
        maybe_in = np.where(T <= ddl[:, None] * (1 + tol_t), sc, np.inf)
        found, n, f, Td, P, E = m.grid_argmin_debug(
            _cu(pc), _cu(lc), _cu(freq), n_max, 0, _cu(ci), _cu(price), True,
            _cu(ddl), fp32)
        assert bool(found.all())
        pick = _pick_index(n.cpu().numpy(), f.cpu().numpy(), n_freq, freq)
        rows = np.arange(len(ddl))
        tol = TOL32 if fp32 else TOL64
        assert np.all(np.isfinite(maybe_in[rows, pick]))
        assert np.all(sc[rows, pick] <= sure_in.min(axis=1) * (1 + tol))


# ------------------------------------------------------------ wave_energy_freq

@gpu
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fp32", (False, True))
@pytest.mark.parametrize("n_freq", (1, 8, 72))
def test_energy_freq_random(build, fp32, n_freq):
    rng = np.random.default_rng(72 + n_freq)
    B = 512
    pc, lc = random_coeffs(rng, B)
    n = rng.integers(1, 9, B).astype(np.int32)
    freq = ladder(n_freq)
    sc = np_job_power(n[:, None], freq[None, :], pc[:, None, :]) * \
        np_unit_time(n[:, None], freq[None, :], lc[:, None, :])
    f = _mod(build).energy_freq_debug(_cu(pc), _cu(lc), _cu(freq), _cu(n),
                                      fp32).cpu().numpy()
    assert np.isin(f, freq).all()
    pick = np.array([int(np.flatnonzero(freq == x)[0]) for x in f])
    exempt = _check_picks(sc, pick, TOL32 if fp32 else TOL64,
                          f"{build} fp32={fp32} n_freq={n_freq}")
    if not fp32:
        assert exempt < 0.01


@gpu
@pytest.mark.parametrize("build", BUILDS)
def test_energy_freq_tie_break_exact(build):
    """At fixed n the score is p(f) * A(f) / n * n: tie_table's classes tie
    frequency 1 (at k1) with 1/2 (at k2); the lower index must win whichever
    lane and pass holds it."""
    m = _mod(build)
    for n_freq, pairs in ((8, ((0, 7), (3, 4))),
                          (72, ((15, 16), (31, 32), (0, 63), (3, 67), (5, 70),
                                (0, 71)))):
        for k1, k2 in pairs:
            for lo, hi in ((k1, k2), (k2, k1)):
                # frequency 1 at `lo`, 1/2 at `hi`: the winner is the lower
                # index, so the expected VALUE flips with the assignment
                pc, lc, freq, _ = tie_table(n_freq, 2, lo, 3, hi)
                for n in (1, 4, 8):
                    sc = np_job_power(np.int64(n), freq, pc) * \
                        np_unit_time(np.int64(n), freq, lc)
                    assert sc[k1] == sc[k2] == sc.min()
                    assert int(np.argmin(sc)) == k1
                    f = m.energy_freq_debug(
                        _cu(pc[None]), _cu(lc[None]), _cu(freq),
                        _cu(np.array([n], dtype=np.int32)), False).item()
                    assert f == freq[k1], (n_freq, k1, k2, lo, hi, n)
    # every frequency ties: the first one
    freq = 2.0 ** -np.arange(72.0)[::-1]
    f = m.energy_freq_debug(_cu(np.array([[0.0, 0.0, 5.0]])),
                            _cu(np.array([[D, 0.0, 0.0]])), _cu(freq),
                            _cu(np.array([4], dtype=np.int32)), False).item()
    assert f == freq[0]
