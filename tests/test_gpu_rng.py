"""GPU tests that pin the device RNG (ops/csrc/hip/philox.hpp) to the host
reference (engine/_philox_host.py, itself pinned to the Random123 vectors and
to mpmath by test_philox_cpu.py).

Four layers, all through debug entry points that run the production device
functions, in both the 64-lane and the 8-lane extension:
  1. philox4x32 word for word;
  2. every production draw from a fresh state at Philox-reached words: one
     counter consumed each, u01 / u01x2 / rbelow bit for bit, the
     transcendental recipes against mpmath;
  3. the word -> value halves of the recipes at chosen edge words;
  4. a finished BatchedEngine run against a host replay of each replica's
     whole random stream (rng_reference.replay_replica).

Tolerances of the transcendental recipes, in ulps of the mpmath value.  The
host column is the largest error of the plain host recipe (math, glibc) over
the rows of layer 3, measured on the CPU and asserted by test_philox_cpu.py;
the device bound is twice that plus 2 ulp (the device library may round each
of the up to two transcendental calls one ulp differently, and exp amplifies
both sides alike).  Neither comes from device output.

    recipe        host    device bound
    rexp          1.24    4.48
    rnormal       0.65    3.30
    rlognormal    8.41    18.82
    rpareto_inf   1.31    4.62
"""
import functools
import math
import types

import numpy as np
import pytest

import rng_reference as R
from distributed_cluster_gpus_amd.engine import _philox_host as ph

torch = pytest.importorskip("torch")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs MI355X")]

BUILDS = ("_sim_hip", "_sim_hip_mw")
SEED = 123          # test_philox_cpu.py checks the replay's conditions for it
M64 = 2 ** 64 - 1


def _mod(name):
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    return load_sim_hip(name)


def _i64(values):
    """python ints as 64-bit patterns -> int64 cuda tensor"""
    a = np.asarray([v & M64 for v in values], dtype=np.uint64).view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


@functools.lru_cache(maxsize=None)
def _key_ctr_rows():
    """(keys, ctrs) as python ints: the zero known-answer vector, the word
    boundaries of key and counter, the engine's replica keys, random rows."""
    edge = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1)
    rows = [(0, 0)]
    rows += [(k, c) for k in edge for c in edge]
    for g in (0, 1, 63, 64, 2 ** 20, 2 ** 31 - 1):
        for c in (0, 16, 2 ** 32 - 1):
            rows.append((ph.replica_key(SEED, g), c))
    rng = np.random.default_rng(4)
    rnd = rng.integers(0, 2 ** 64, size=(512 - len(rows), 2), dtype=np.uint64)
    rows += [(int(k), int(c)) for k, c in rnd]
    assert len(rows) == 512
    return tuple(rows)


# ---------------------------------------------------------------- layer 1

@pytest.mark.parametrize("build", BUILDS)
def test_philox_words_equal_host(build):
    rows = _key_ctr_rows()
    got = _mod(build).philox_debug(_i64([k for k, _ in rows]),
                                   _i64([c for _, c in rows])).cpu().tolist()
    assert tuple(got[0]) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    for (k, c), w in zip(rows, got):
        assert tuple(w) == ph.philox4x32(k, c), (hex(k), hex(c))


# ---------------------------------------------------------------- layer 2

@pytest.mark.parametrize("build", BUILDS)
def test_draws_at_philox_words(build):
    rows = _key_ctr_rows()
    n_below = [(1, 8, 2 ** 32 - 1, 8)[i % 4] for i in range(len(rows))]
    vals, below, after = _mod(build).rng_draws_debug(
        _i64([k for k, _ in rows]), _i64([c for _, c in rows]),
        _i64(n_below), R.LAMBD, R.MU, R.SIGMA)
    vals = vals.cpu().numpy()
    below = below.cpu().tolist()
    after = [[v & M64 for v in row] for row in after.cpu().tolist()]
    worst = dict.fromkeys(R.RECIPES, 0.0)
    for i, (k, c) in enumerate(rows):
        # every draw takes exactly one counter
        assert after[i] == [(c + 1) & M64] * 7, (hex(k), hex(c))
        ua, ub = ph.philox_u01_pair(k, c)
        # exact arithmetic: bit for bit
        assert vals[i, 0].tobytes() == np.float64(ua).tobytes()
        assert vals[i, 1].tobytes() == np.float64(ua).tobytes()
        assert vals[i, 2].tobytes() == np.float64(ub).tobytes()
        assert below[i] == ph.rbelow(k, c, n_below[i]) < n_below[i]
        ref = {"rexp": R.mp_rexp(ua), "rnormal": R.mp_rnormal(ua, ub),
               "rlognormal": R.mp_rlognormal(ua, ub),
               "rpareto_inf": R.mp_rpareto_inf(ua)}
        for col, recipe in zip((3, 4, 5, 6), R.RECIPES):
            worst[recipe] = max(worst[recipe],
                                R.ulp_error(float(vals[i, col]), ref[recipe]))
    for recipe in R.RECIPES:
        print(f"{build} {recipe}: device max error {worst[recipe]:.3f} ulp, "
              f"bound {R.device_bound(recipe):.2f}")
    for recipe in R.RECIPES:
        assert worst[recipe] <= R.device_bound(recipe), recipe


# ---------------------------------------------------------------- layer 3

@functools.lru_cache(maxsize=None)
def _maps(build):
    words, n_below = R.word_rows()
    vals, below = _mod(build).rng_maps_debug(
        torch.from_numpy(words.copy()).cuda(),
        torch.from_numpy(n_below.copy()).cuda(), R.LAMBD, R.MU, R.SIGMA)
    return vals.cpu().numpy(), below.cpu().tolist()


@pytest.mark.parametrize("build", BUILDS)
def test_maps_exact_parts(build):
    vals, below = _maps(build)
    words, n_below = R.word_rows()
    for i, (ua, ub) in enumerate(R.uniforms()):
        assert vals[i, 0].tobytes() == np.float64(ua).tobytes()
        assert vals[i, 2].tobytes() == np.float64(ub).tobytes()
        assert below[i] == ph.rbelow_map(int(words[i, 0]), int(n_below[i]))
        assert 0 <= below[i] < n_below[i]
    z, o = R.edge_index("zero"), R.edge_index("ones")
    assert vals[z, 0] == 0.0 and not np.signbit(vals[z, 0])
    assert vals[o, 0] == R.U_MAX and vals[o, 0] != 1.0
    assert vals[R.edge_index("dropped bits"), 0] == 0.0
    for n in (1, 8, 2 ** 32 - 1):
        i = R.edge_index(f"rbelow n={n}")
        assert words[i, 0] == R.W_MAX and below[i] == n - 1


@pytest.mark.parametrize("build", BUILDS)
def test_maps_edges(build):
    vals, _ = _maps(build)
    z, o = R.edge_index("zero"), R.edge_index("ones")
    # rexp at u = 0: a zero of either sign that leaves the clock alone
    assert vals[z, 3] == 0.0
    for now in (0.0, 17.25, 604800.0):
        assert now + vals[z, 3] == now
    assert np.isfinite(vals[o, 3]) and vals[o, 3] > 0
    # Box-Muller corners
    for name, _, _ in R.EDGE_ROWS:
        if name.startswith("bm "):
            i = R.edge_index(name)
            assert np.isfinite(vals[i, 4]) and np.isfinite(vals[i, 5]), name
    # Pareto: u01 = 0 gives the scale itself; the clamp gives the largest size
    assert vals[z, 6] == 1.0
    cap_mp = R.MP.power(R.MP.mpf(1e-9), -R.MP.mpf(1.0 / 1.8))
    cap = vals[o, 6]
    assert R.ulp_error(float(cap), cap_mp) <= R.device_bound("rpareto_inf")
    assert vals[R.edge_index("pareto 1-u=9007199*2^-53"), 6] == cap
    assert vals[R.edge_index("pareto 1-u=1*2^-53"), 6] == cap
    assert vals[R.edge_index("pareto 1-u=9007200*2^-53"), 6] < cap
    assert vals[:, 6].max() == cap


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("recipe", R.RECIPES)
def test_maps_against_mpmath(build, recipe):
    vals, _ = _maps(build)
    col = 3 + R.RECIPES.index(recipe)
    err = R.max_ulp_error(vals[:, col], recipe)
    print(f"{build} {recipe}: device max error {err:.3f} ulp, host table "
          f"{R.HOST_MAX_ULP[recipe]}, bound {R.device_bound(recipe):.2f}")
    assert err <= R.device_bound(recipe)


# ---------------------------------------------------------------- layer 4

END = 30.0
CASES = {
    # name: (algo, Poisson inference?, replicas, rank, world, engine kwargs)
    "paper": ("default_policy", False, 8, 0, 1, {}),
    "paper_short_launches": ("default_policy", False, 8, 0, 1,
                             {"events_per_launch": 500}),
    "eco_route_poisson": ("eco_route", True, 8, 0, 1, {}),
    "world3_rank2": ("default_policy", False, 24, 2, 3, {}),
}


def _arrivals(poisson_inf):
    from distributed_cluster_gpus_amd.configs.paper import build_arrivals
    return build_arrivals(inf_mode="poisson") if poisson_inf \
        else build_arrivals()


@functools.lru_cache(maxsize=None)
def _replays(algo, poisson_inf, replicas, rank, world):
    """The host replay of every replica of the shard; computed once per
    distinct stream set and shared."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.parallel.sharding import replica_shard
    sc = paper_scenario()
    arrs = _arrivals(poisson_inf)
    shard = replica_shard(replicas, rank, world)
    first = BatchedEngine._seed_arrivals(types.SimpleNamespace(sc=sc),
                                         arrs[0], arrs[1], SEED, shard)
    reps = [R.replay_replica(SEED, shard.start + r, first[r], arrs, sc.n_dc,
                             END, draws_dc=algo != "eco_route")
            for r in range(shard.count)]
    return shard, first, tuple(reps)


@pytest.mark.parametrize("case", list(CASES))
def test_whole_stream_replay(case):
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    algo, poisson_inf, replicas, rank, world, kw = CASES[case]
    shard, first, reps = _replays(algo, poisson_inf, replicas, rank, world)
    if case == "world3_rank2":
        assert (shard.start, shard.count) == (16, 8)
    # the replay's own conditions: an ulp can neither reorder two arrivals
    # nor flip a thinning acceptance
    assert min(rep.min_gap for rep in reps) > 1e-9
    assert min(rep.min_margin for rep in reps) > 1e-12

    arrs = _arrivals(poisson_inf)
    eng = BatchedEngine(paper_scenario(), arrs[0], arrs[1], algo=algo,
                        replicas=replicas, duration=END, log_interval=5.0,
                        out_dir=None, seed=SEED, enable_logs=True,
                        rank=rank, world=world, **kw)
    eng.run()
    t = eng.t
    assert int(t["done"].min().item()) == 1
    ns = first.shape[1]

    # counters: exactly
    assert t["rng_ctr"].cpu().tolist() == [rep.ctr for rep in reps]
    assert t["jid_ctr"].cpu().tolist() == [rep.jid for rep in reps]
    assert all(rep.ctr > ns for rep in reps)

    # next arrival per stream
    arr_next = t["arr_next"].cpu().numpy()
    b_rexp = R.device_bound("rexp")
    for r, rep in enumerate(reps):
        for s in range(ns):
            tol = rep.n_arrivals[s] * b_rexp * math.ulp(END)
            assert abs(arr_next[r, s] - rep.arr_next[s]) <= tol, (r, s)
            assert arr_next[r, s] > END

    # every job still running at the end, on every replica, joined on jid
    # (30 s finish no training job, so these carry the lognormal sizes).
    # SRec is 64 bytes: size is f64 #2, jid the int32 at byte 44 (seq follows), ing the
    # byte at 52.
    s_rec = t["s_rec"].cpu().numpy()
    s_jid = s_rec.view(np.int32).reshape(s_rec.shape[:2] + (16,))[..., 11]
    s_ing = s_rec.view(np.uint8).reshape(s_rec.shape[:2] + (64,))[..., 52]
    running = t["s_gpus"].cpu().numpy() > 0
    s_jt = t["s_jtype"].cpu().numpy()
    worst = {0: 0.0, 1: 0.0}
    count = {0: 0, 1: 0}
    for r, slot in zip(*np.nonzero(running)):
        if s_jid[r, slot] == 0 and r != eng.log_replica:
            continue    # went through a queue: only the log replica's queues
                        # carry the jid along
        ing, jt, _, _, size_mp = reps[r].jobs[int(s_jid[r, slot])]
        assert (int(s_ing[r, slot]), int(s_jt[r, slot])) == (ing, jt)
        worst[jt] = max(worst[jt],
                        R.ulp_error(float(s_rec[r, slot, 2]), size_mp))
        count[jt] += 1
    print(f"{case}: {count[0]} + {count[1]} running jobs, size error "
          f"{worst[0]:.3f} ulp (pareto), {worst[1]:.3f} ulp (lognormal)")
    assert count[1] >= 8
    assert worst[0] <= R.device_bound("rpareto_inf")
    assert worst[1] <= R.device_bound("rlognormal")

    # the logging replica's job log, joined on jid
    if shard.start != 0:
        assert eng.log_replica < 0
        # the key is the GLOBAL id: the same shard replayed under its local
        # ids does not even consume the same number of counters
        local = R.replay_replica(SEED, 0, first[0], arrs, 8, END)
        assert local.ctr != reps[0].ctr
        return
    assert eng.log_replica == 0
    chunks = list(eng._jl_chunks)
    n_jl = int(t["jl_count"].item())
    if n_jl:
        chunks.append(t["jl_rows"][:n_jl].cpu().numpy())
    rows = np.concatenate(chunks, axis=0)
    jobs = reps[0].jobs
    assert len(rows) > len(jobs) // 2
    assert len(set(rows[:, 0].tolist())) == len(rows)
    worst = {0: 0.0, 1: 0.0}
    assert len(rows) > 500
    for row in rows:
        ing, jt, dc, _, size_mp = jobs[int(row[0])]
        assert (int(row[1]), int(row[2])) == (ing, jt)
        if dc is not None:      # eco_route scores the DC, it does not draw it
            assert int(row[4]) == dc
        worst[jt] = max(worst[jt], R.ulp_error(float(row[3]), size_mp))
    print(f"{case}: {len(rows)} logged jobs, size error {worst[0]:.3f} ulp "
          f"(pareto), {worst[1]:.3f} ulp (lognormal)")
    assert worst[0] <= R.device_bound("rpareto_inf")
    assert worst[1] <= R.device_bound("rlognormal")
