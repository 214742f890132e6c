"""Per-ingress arrival rate profiles on the device: pregen_arrivals_kernel's
PROF instantiations (ops/csrc/hip/arrival_ring.hpp).

Function level, the production profile_gap is bitwise the host twin
(models/arrivals.py) on the same E.  Engine level, a host replay walks every
replica's merged streams with the twin and the host Philox: counters and
arrival counts must match exactly, next-arrival times within the error the
device's log may add.  The ring mechanics, sharding and sweeps of the other
modes are repeated in profile mode, and the batched population is compared
with the native engine's.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import profile_reference as pr  # noqa: E402
from rng_reference import device_bound  # noqa: E402
from distributed_cluster_gpus_amd.engine import _philox_host as ph  # noqa: E402
from distributed_cluster_gpus_amd.models.arrivals import (  # noqa: E402
    ArrivalProcess, profile_gap)

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="needs a ROCm GPU")

RING = {"arr_ring", "arr_head", "arr_count", "gen_arr_next", "gen_ctr",
        "arr_more"}
SEED = 123
ZERO_ROW = 3          # the ingress whose inference row is all zero
D_INF = ph.D_INF


def _arrivals(mixed=False):
    inf, trn = pr.paper_profiles(zero_row=ZERO_ROW)
    if mixed:
        trn = ArrivalProcess(mode="poisson", rate=0.3)
    return inf, trn


def _engine(*, arrivals=None, **over):
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    inf, trn = arrivals or _arrivals()
    kw = dict(algo="default_policy", replicas=6, duration=pr.DURATION,
              log_interval=5.0, out_dir=None, enable_logs=False, seed=SEED)
    kw.update(over)
    return BatchedEngine(paper_scenario(), inf, trn, **kw)


def _sim_mod():
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    return load_sim_hip("_sim_hip")


# ------------------------------------------------------------ function level

def _table(rows):
    """arr_prof rows (engine/state.py profile_table's layout) of the given
    multiplier rows, one stream each."""
    from distributed_cluster_gpus_amd.engine.state import PROF_SEG, PROF_W
    tab = np.zeros((len(rows), PROF_W))
    for s, row in enumerate(rows):
        m, cum = pr.tables(row)
        tab[s, 0] = len(m)
        tab[s, 1:1 + len(m)] = m
        tab[s, 1 + PROF_SEG:2 + PROF_SEG + len(m)] = cum
    return tab


def _device_gaps(E, t, stream, rate, period, tab):
    dev = torch.device("cuda")
    out = _sim_mod().profile_gap_debug(
        torch.tensor(E, dtype=torch.float64, device=dev),
        torch.tensor(t, dtype=torch.float64, device=dev),
        torch.tensor(stream, dtype=torch.int32, device=dev),
        float(rate), float(period),
        torch.tensor(tab, dtype=torch.float64, device=dev))
    return out.cpu().numpy()


def _assert_bitwise(got, want, what):
    got = np.asarray(got, np.float64).view(np.int64)
    want = np.asarray(want, np.float64).view(np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, bad[:5].tolist(),
                           got[bad[:5]].view(np.float64).tolist(),
                           want[bad[:5]].view(np.float64).tolist())


@needs_gpu
def test_profile_gap_edge_cases_bitwise():
    """the CPU edge cases, and the two off cases, one stream per case"""
    cases = pr.EDGE_ROWS + pr.OFF_ROWS
    tab = _table([c[1] for c in cases])
    by_params = {}
    for s, (_, m, rate, period, t, E) in enumerate(cases):
        by_params.setdefault((rate, period), []).append((s, m, t, E))
    for (rate, period), rows in by_params.items():
        got = _device_gaps([r[3] for r in rows], [r[2] for r in rows],
                           [r[0] for r in rows], rate, period, tab)
        want = [profile_gap(E, t, rate, period, *pr.tables(m))
                for _, m, t, E in rows]
        _assert_bitwise(got, want, (rate, period))
    off = [s for s, c in enumerate(cases) if c in pr.OFF_ROWS]
    assert len(off) == 2


@needs_gpu
@pytest.mark.parametrize("K", [5, 64])
def test_profile_gap_random_rows_bitwise(K):
    """256 rows over all 16 streams of a table: K = 5 is no multiple of the
    group's 8 lanes, K = 64 takes all eight search steps"""
    rng = np.random.default_rng(950 + K)
    if K == 5:
        rows = [r for pair in zip(pr.rotations(pr.BASE_INF),
                                  pr.rotations(pr.BASE_TRN)) for r in pair]
    else:
        rows = rng.uniform(0.0, 3.0, (16, 64))
        rows[rng.random((16, 64)) < 0.3] = 0.0
        rows[:, 63] = np.where(np.arange(16) % 2, rows[:, 63], 0.5)
        rows = list(rows)
    tab = _table(rows)
    B = 256
    stream = (np.arange(B) % 16).astype(np.int32)
    period, rate = 120.0, 1.5
    t = rng.uniform(0.0, 6.0 * period, B)
    t[:16] = np.arange(16) * (period / K)          # on segment boundaries
    t[16:32] = period * np.arange(16)              # on cycle boundaries
    E = rng.exponential(1.0, B) * rng.choice([1e-9, 1.0, 1.0, 300.0], B)
    E[32:40] = 0.0
    got = _device_gaps(E, t, stream, rate, period, tab)
    want = [profile_gap(float(E[i]), float(t[i]), rate, period,
                        *pr.tables(rows[stream[i]])) for i in range(B)]
    _assert_bitwise(got, want, f"K={K}")
    assert np.isfinite(got).all() and (got >= 0).all()


# -------------------------------------------------------------------- replay

class Replay:
    def __init__(self, ns):
        self.ctr = ns
        self.jid = 0
        self.arr_next = None
        self.bound = [0.0] * ns       # device error bound of arr_next[s]
        self.n_arrivals = [0] * ns
        self.draws = [0] * ns         # gap draws the stream consumed


def replay_replica(seed, global_id, arrivals, n_ing, end_time, draws_dc=True):
    """One replica's merged arrival streams to end_time, by the twin: the
    seed draws of engine/batched.py seed_arrivals, then per arrival the size
    draw, the route draw and the gap (one draw in profile mode, one for
    Poisson).  Per stream, the bound on what the device's log may move its
    next arrival: sum over its arrivals of device_bound(rexp) * ulp(E) /
    (rate * m at the landing segment) + 4 ulp(t).  Asserts its own
    preconditions: no two candidate times, and no candidate and segment
    boundary, closer than that bound (so that no perturbation within it
    reorders the merge or changes a landing segment)."""
    key = ph.replica_key(seed, global_id)
    ns = 2 * n_ing
    out = Replay(ns)
    db = device_bound("rexp")

    def gap(s, ctr, t):
        """(ia, counter after, bound of t + ia given E's error)"""
        a = arrivals[s & 1]
        if a.mode == "profile":
            m, cum = a._table(s >> 1)
            if not (a.rate > 0 and cum[-1] > 0):
                return D_INF, ctr, 0.0
            E = ph.rexp_map(ph.philox_u01(key, ctr), 1.0)
            g = profile_gap(E, t, a.rate, a.period, m, cum)
            K = len(m)
            k = min(K - 1, int(math.fmod(t + g, a.period) / a.period * K))
            # a landing exactly on the start of segment k belongs to k - 1's
            # end only for E = 0; m[k] > 0 by construction of the inversion
            lam = a.rate * (m[k] if m[k] > 0 else max(m))
            return g, ctr + 1, db * math.ulp(E) / lam + 4 * math.ulp(t + g)
        assert a.mode in ("poisson", "off")
        ia, c2 = ph.draw_interarrival(key, ctr, t, a.mode, a.rate)
        if ia >= D_INF:
            return D_INF, c2, 0.0
        return ia, c2, db * math.ulp(ia) + 4 * math.ulp(t + ia)

    nxt = []
    for s in range(ns):                       # the seed draws: ctr = s, t = 0
        ia, _, b = gap(s, s, 0.0)
        nxt.append(ia if ia < D_INF else 1e300)
        out.bound[s] = b
    first = list(nxt)
    while True:
        order = sorted(range(ns), key=lambda k: (nxt[k], k))
        s = order[0]
        t = nxt[s]
        if t > end_time:
            break
        # preconditions at this candidate
        s2 = order[1]
        if nxt[s2] < D_INF:
            assert nxt[s2] - t > out.bound[s] + out.bound[s2], \
                ("two candidates too close", global_id, s, s2, t, nxt[s2])
        a = arrivals[s & 1]
        if a.mode == "profile":
            seg = a.period / a.profile.shape[1]
            d = math.fmod(t, seg)
            assert min(d, seg - d) > out.bound[s], \
                ("candidate on a segment boundary", global_id, s, t)
        assert abs(end_time - t) > out.bound[s]
        out.jid += 1
        out.n_arrivals[s] += 1
        out.ctr += 2 if draws_dc else 1       # size, route
        ia, out.ctr, b = gap(s, out.ctr, t)
        out.draws[s] += 1 if ia < D_INF else 0
        nxt[s] = t + ia if ia < D_INF else 1e300
        out.bound[s] += b
    for s in range(ns):                       # ... and against end_time
        if nxt[s] < D_INF:
            assert nxt[s] - end_time > out.bound[s]
    out.arr_next = nxt
    out.first = first
    return out


@functools.lru_cache(maxsize=None)
def _replays(n, mixed=False, end_time=pr.DURATION):
    return tuple(replay_replica(SEED, r, _arrivals(mixed), pr.N_ING, end_time)
                 for r in range(n))


@functools.lru_cache(maxsize=None)
def _finished(replicas, mixed=False):
    """a finished default_policy run of the paper scenario; tests only read"""
    eng = _engine(arrivals=_arrivals(mixed), replicas=replicas)
    seeded = eng.t["arr_next"].cpu().numpy().copy()
    eng.run()
    assert int(eng.t["err"].max()) == 0 and bool((eng.t["done"] == 1).all())
    return eng, seeded


def _check_against_replay(eng, seeded, reps):
    R = len(reps)
    ctr = eng.t["rng_ctr"].cpu().numpy()
    jid = eng.t["jid_ctr"].cpu().numpy()
    nxt = eng.t["arr_next"].cpu().numpy()
    worst = 0.0
    for r, rep in enumerate(reps):
        # the seeds are the twin's own (host), bit for bit
        assert seeded[r].tolist() == rep.first, r
        assert int(ctr[r]) == rep.ctr, (r, int(ctr[r]), rep.ctr)
        assert int(jid[r]) == rep.jid, (r, int(jid[r]), rep.jid)
        for s in range(nxt.shape[1]):
            want = rep.arr_next[s]
            if want >= D_INF:
                assert nxt[r, s] == D_INF, (r, s)
                continue
            err = abs(nxt[r, s] - want)
            assert err <= rep.bound[s], (r, s, nxt[r, s], want, rep.bound[s])
            worst = max(worst, err / rep.bound[s])
    print(f"{R} replicas: worst arr_next error {worst:.3g} of its bound")


@needs_gpu
@pytest.mark.parametrize("replicas", [6, 70])
def test_replay(replicas):
    """6 replicas: part of one generator wave; 70: three blocks of 32 groups,
    tail lanes and a part-filled last wave"""
    eng, seeded = _finished(replicas)
    assert "arr_prof" in eng.t and eng._sim.arrival_pregen()
    _check_against_replay(eng, seeded, _replays(70)[:replicas])


@needs_gpu
def test_segment_totals_on_the_device():
    """every arrival the replay counts is somewhere on the device: finished,
    queued, running or in transfer; the all-zero row's stream never fires"""
    eng, seeded = _finished(70)
    t = eng.t
    held = (t["jobs_done"] + t["q_len"].sum(dim=(1, 2)) +
            t["n_running"].sum(dim=1) +
            (t["x_time"] < D_INF).sum(dim=1)).cpu().numpy()
    reps = _replays(70)
    assert held.tolist() == [rep.jid for rep in reps]
    off = 2 * ZERO_ROW
    assert (seeded[:, off] == D_INF).all()
    assert bool((t["arr_next"][:, off] == D_INF).all())
    assert bool((t["gen_arr_next"][:, off] == D_INF).all())
    assert all(rep.n_arrivals[off] == 0 for rep in reps)
    assert min(rep.n_arrivals[off + 1] for rep in reps) > 0


# ------------------------------------------------------------ ring mechanics

def _same(a, b, what, skip=RING):
    torch.cuda.synchronize()
    for k in a.t:
        if k in skip:
            continue
        x, y = a.t[k], b.t[k]
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), f"{what}: {k}"
    assert int(a.t["err"].max()) == 0 and int(b.t["err"].max()) == 0, what


def _calls(a, b, calls, what="", skip=RING):
    for i, (t_target, E) in enumerate(calls):
        a._sim.advance(float(t_target), E)
        b._sim.advance(float(t_target), E)
        _same(a, b, f"{what} call {i} ({t_target}, {E})", skip)


def _events(eng):
    return int(eng.t["ev_count"].sum().item())


@needs_gpu
def test_wrap_and_substeps():
    """arr_cap = 8: a call of 100 events is 13 sub-steps and the ring wraps
    many times; nothing outside the ring may differ from the roomy ring's"""
    small = _engine(replicas=5, arr_cap=8, duration=60.0)
    roomy = _engine(replicas=5, duration=60.0)
    plan = small._sim.launch_plan(100)
    assert len(plan) == 13 and sum(w[3] for w in plan) == 100
    assert len(roomy._sim.launch_plan(100)) == 1
    _calls(small, roomy, [(60.0, 100)] * 6)
    assert _events(small) == 5 * 600
    off = 2 * ZERO_ROW
    assert bool((small.t["arr_next"][:, off] == D_INF).all())


@needs_gpu
def test_forced_windows():
    """6 replicas under set_launch_plan(4, 8, 1, 0): every sub-step is three
    windows, the middle one with two budgets"""
    win, one = _engine(duration=60.0), _engine(duration=60.0)
    win._sim.set_launch_plan(4, 8, 1, 0)
    plan = win._sim.launch_plan(300)
    assert len(plan) == 3 and any(w[2] < w[1] for w in plan)
    assert len(one._sim.launch_plan(300)) == 1
    _calls(win, one, [(60.0, 300)] * 3, skip=set())
    assert _events(win) == 6 * 900


@needs_gpu
def test_checkpoint_with_a_non_empty_ring(tmp_path):
    on, ref = (_engine(arr_cap=256, duration=60.0) for _ in range(2))
    _calls(on, ref, [(60.0, 200)] * 2, skip=set())
    assert int(on.t["arr_count"].min()) > 0      # records left in the ring
    path = str(tmp_path / "mid.pt")
    on.save_state(path)
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert torch.equal(saved["tensors"]["arr_prof"], on.t["arr_prof"].cpu())
    resumed = _engine(arr_cap=256, duration=60.0)
    resumed.load_state(path)
    for i in range(3):
        ref._sim.advance(60.0, 200)               # the uninterrupted run
        resumed._sim.advance(60.0, 200)
        _same(resumed, ref, f"after load {i}", skip=set())
    assert _events(resumed) == 6 * 1000
    # another table's checkpoint is refused
    other = _engine(arr_cap=256, duration=60.0,
                    arrivals=pr.paper_profiles(zero_row=5))
    with pytest.raises(ValueError, match="arr_prof"):
        other.load_state(path)


# ------------------------------------------------------- sharding and sweeps

def _rows_equal(whole, part, a, b, what):
    torch.cuda.synchronize()
    compared = 0
    for k in part.t:
        x, y = whole.t[k], part.t[k]
        if tuple(x.shape) == tuple(y.shape):
            continue                         # not replica-leading
        assert x.shape[0] == whole.R, k
        x = x[a:b]
        if x.dtype == torch.float64:
            x, y = (z.contiguous().view(torch.int64) for z in (x, y))
        assert torch.equal(x, y), f"{what}: {k}"
        compared += 1
    assert compared >= 40
    assert int(part.t["err"].max()) == 0 and int(whole.t["err"].max()) == 0


TO_END = [(60.0, 300)] * 3 + [(61.0, 10 ** 9)]


@needs_gpu
def test_sharding():
    whole = _engine(replicas=24, duration=60.0)
    part = _engine(replicas=24, world=3, rank=2, duration=60.0)
    assert (part.shard.start, part.shard.end) == (16, 24)
    for i, (t_target, E) in enumerate(TO_END):
        whole._sim.advance(t_target, E)
        part._sim.advance(t_target, E)
        _rows_equal(whole, part, 16, 24, f"call {i}")
    assert bool((whole.t["done"] == 1).all())


@needs_gpu
def test_sweep_rate_and_period():
    """3 groups x 8 replicas over the inference rate (0.5x, 1x, 2x) and
    period: the SWP, PROF generator; each group is bit for bit the matching
    shard of a uniform profile-mode run at its point"""
    import dataclasses

    from distributed_cluster_gpus_amd.engine.sweep import Sweep
    points = [(0.5 * pr.RATE_INF, 60.0), (pr.RATE_INF, 120.0),
              (2.0 * pr.RATE_INF, 240.0)]
    sweep = Sweep.points([dict(inf_rate=r, inf_period=p) for r, p in points])
    eng = _engine(sweep=sweep, replicas=24, duration=60.0)
    assert {"sw_arr", "arr_prof"} <= set(eng.t)
    inf, trn = _arrivals()
    unis = [_engine(arrivals=(dataclasses.replace(inf, rate=r, period=p), trn),
                    replicas=24, world=3, rank=g, duration=60.0)
            for g, (r, p) in enumerate(points)]
    for i, (t_target, E) in enumerate(TO_END):
        for e in [eng] + unis:
            e._sim.advance(t_target, E)
        for g, u in enumerate(unis):
            a, b = sweep.slice_of(g, eng.shard)
            assert (a, b) == (8 * g, 8 * g + 8)
            _rows_equal(eng, u, a, b, f"call {i} group {g}")
    jobs = [eng.t["jobs_done"][8 * g:8 * g + 8].sum().item() for g in range(3)]
    assert jobs[0] < jobs[1] < jobs[2], jobs
    with pytest.raises(ValueError, match=r"inf_amp.*'profile'"):
        _engine(sweep=Sweep.grid(inf_amp=[0.1, 0.2, 0.3]), replicas=24)


# ------------------------------------------------- mixed modes and neutrality

@needs_gpu
def test_mixed_modes():
    """inference in profile mode, training Poisson: the training streams'
    next arrivals and the draws they consumed are the replay's"""
    eng, seeded = _finished(6, mixed=True)
    reps = _replays(6, mixed=True)
    _check_against_replay(eng, seeded, reps)
    assert min(sum(rep.draws[1::2]) for rep in reps) > 0
    assert min(sum(rep.draws[0::2]) for rep in reps) > 0


@needs_gpu
def test_other_modes_have_no_table():
    from distributed_cluster_gpus_amd.configs.paper import build_arrivals
    eng = _engine(arrivals=build_arrivals(), duration=30.0)
    assert eng.arrival_inf.mode == "sinusoid" and "arr_prof" not in eng.t
    assert "arr_prof" not in [n for n, _, _ in eng._sim.contract()]
    eng.run()
    assert int(eng.t["err"].max()) == 0 and _events(eng) > 0


# ---------------------------------------------------------- population check

@needs_gpu
def test_distributional_match_vs_native():
    """batched against native in profile mode, as test_gpu_engine.py does for
    the default workload: 256 replicas against 10 seeds, 120 s; jobs and
    energy within 4 combined standard errors"""
    import tempfile

    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.native import NativeEngine
    duration = 120.0
    inf, trn = _arrivals()
    nat = []
    for s in range(10):
        with tempfile.TemporaryDirectory() as td:
            nat.append(NativeEngine(paper_scenario(), inf, trn,
                                    algo="default_policy", duration=duration,
                                    log_interval=5.0, out_dir=td, seed=s).run())
    nat_energy = np.array([r["total_energy_j"] for r in nat])
    nat_jobs = np.array([r["jobs_completed"] for r in nat], float)
    eng = _engine(replicas=256, duration=duration)
    eng.run()
    gpu_energy = eng.t["energy_j"].sum(dim=1).cpu().numpy()
    gpu_jobs = eng.t["jobs_done"].cpu().numpy().astype(float)
    for g, n, name in ((gpu_energy, nat_energy, "energy"),
                       (gpu_jobs, nat_jobs, "jobs")):
        se = math.sqrt(n.std() ** 2 / len(n) + g.std() ** 2 / len(g))
        print(f"{name}: gpu {g.mean():.6g} vs native {n.mean():.6g} "
              f"(se {se:.3g})")
        assert abs(g.mean() - n.mean()) < 4 * se + 1e-9, name
