"""Host reference of the device RNG (engine/_philox_host.py), pinned on the
CPU: philox4x32 to the Random123 known-answer vectors, every distribution
recipe to mpmath at 120 bits on the word rows that test_gpu_rng.py feeds the
device (tests/rng_reference.py), the seed draw of BatchedEngine to the
recipes, and the self-conditions of the whole-stream replay.

Largest error of the host recipes over those rows, in ulps of the result
(rng_reference.HOST_MAX_ULP, asserted below):

    recipe        host (math, glibc)
    rexp          1.24
    rnormal       0.65
    rlognormal    8.41   (exp amplifies the ~1 ulp of its argument ~ 10.8)
    rpareto_inf   1.31
"""
import math
import types
from fractions import Fraction

import pytest

import rng_reference as R
from distributed_cluster_gpus_amd.engine import _philox_host as ph

# Random123 kat_vectors, philox4x32 10: counter words, key words, output
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2,
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    k = key[0] | key[1] << 32
    c = ctr[0] | ctr[1] << 32
    assert ph.philox4x32(k, c, ctr[2], ctr[3]) == want


def test_upper_counter_words_default_to_zero():
    for key, ctr in ((0, 0), (123, 16), (2 ** 64 - 1, 2 ** 63), (7, 2 ** 32)):
        assert ph.philox4x32(key, ctr) == ph.philox4x32(key, ctr, 0, 0)
    # and they matter, each on its own
    base = ph.philox4x32(5, 9)
    assert ph.philox4x32(5, 9, 1, 0) != base
    assert ph.philox4x32(5, 9, 0, 1) != base
    assert ph.philox4x32(5, 9, 1, 0) != ph.philox4x32(5, 9, 0, 1)
    # a counter is read as two words: word 1 is not dropped or folded
    assert ph.philox4x32(5, 2 ** 32) != ph.philox4x32(5, 0)
    assert ph.philox4x32(5, 2 ** 32) != ph.philox4x32(5, 1)


def test_replica_key():
    assert ph.replica_key(123, 0) == 123
    assert ph.replica_key(0, 1) == 0x9E3779B97F4A7C15
    assert ph.replica_key(0, 2) == (2 * 0x9E3779B97F4A7C15) % 2 ** 64
    g = 2 ** 31 - 1
    assert ph.replica_key(123, g) == 123 ^ ((0x9E3779B97F4A7C15 * g) % 2 ** 64)
    keys = {ph.replica_key(123, g) for g in range(4096)}
    assert len(keys) == 4096


def test_u01_and_rbelow_are_exact():
    words, n_below = R.word_rows()
    for w, n in zip(words.tolist(), n_below.tolist()):
        u = ph.u01_map(w[0], w[1])
        assert Fraction(u) == Fraction((w[0] >> 5) * 2 ** 26 + (w[1] >> 6),
                                       2 ** 53)
        assert 0.0 <= u < 1.0
        b = ph.rbelow_map(w[0], n)
        assert b == w[0] * n // 2 ** 32 and 0 <= b < n


def test_recipe_edges_host():
    hv, us = R.host_values(), R.uniforms()
    z, o = R.edge_index("zero"), R.edge_index("ones")
    assert us[z] == (0.0, 0.0)
    assert us[o] == (R.U_MAX, R.U_MAX) and R.U_MAX < 1.0
    assert us[R.edge_index("dropped bits")] == (0.0, 0.0)
    assert us[R.edge_index("lowest kept bits")] == (2.0 ** -27 + 2.0 ** -53,) * 2
    assert us[R.edge_index("bm ua=0 ub=1/4")] == (0.0, 0.25)
    assert us[R.edge_index("bm ua=max ub=1/2")] == (R.U_MAX, 0.5)
    # rexp: u = 0 gives a zero that leaves the clock where it is
    assert hv["rexp"][z] == 0.0 and 17.25 + hv["rexp"][z] == 17.25
    assert math.isfinite(hv["rexp"][o]) and hv["rexp"][o] > 0
    for name, _, _ in R.EDGE_ROWS:
        if name.startswith("bm "):
            i = R.edge_index(name)
            assert math.isfinite(hv["rnormal"][i])
            assert math.isfinite(hv["rlognormal"][i])
    assert hv["rpareto_inf"][z] == 1.0
    # the clamp: everything with 1 - u01 < 1e-9 gives the largest job size
    cap = hv["rpareto_inf"][o]
    assert hv["rpareto_inf"][R.edge_index("pareto 1-u=9007199*2^-53")] == cap
    assert hv["rpareto_inf"][R.edge_index("pareto 1-u=1*2^-53")] == cap
    assert hv["rpareto_inf"][R.edge_index("pareto 1-u=9007200*2^-53")] < cap
    assert max(hv["rpareto_inf"]) == cap
    assert R.ulp_error(cap, R.MP.power(R.MP.mpf(1e-9),
                                       -R.MP.mpf(1.0 / 1.8))) <= 1.31


@pytest.mark.parametrize("recipe", R.RECIPES)
def test_host_recipe_against_mpmath(recipe):
    assert R.MP.prec >= 100
    err = R.max_ulp_error(R.host_values()[recipe], recipe)
    print(f"{recipe}: host max error {err:.3f} ulp "
          f"(table {R.HOST_MAX_ULP[recipe]}, device bound "
          f"{R.device_bound(recipe):.2f})")
    assert err <= R.HOST_MAX_ULP[recipe]


def test_draws_consume_one_counter_and_match_their_maps():
    key = ph.replica_key(123, 5)
    for ctr in (0, 16, 2 ** 32 - 1, 2 ** 32):
        w = ph.philox4x32(key, ctr)
        ua, ub = ph.u01_map(w[0], w[1]), ph.u01_map(w[2], w[3])
        assert ph.philox_u01(key, ctr) == ua
        assert ph.philox_u01_pair(key, ctr) == (ua, ub)
        assert ph.rexp(key, ctr, R.LAMBD) == ph.rexp_map(ua, R.LAMBD)
        assert ph.rbelow(key, ctr, 8) == ph.rbelow_map(w[0], 8)
        assert ph.rnormal(key, ctr, R.MU, 0.4) == ph.rnormal_map(ua, ub, R.MU, 0.4)
        assert ph.rlognormal(key, ctr, R.MU, 0.4) == \
            ph.rlognormal_map(ua, ub, R.MU, 0.4)
        assert ph.rpareto_inf(key, ctr) == ph.rpareto_inf_map(ua)


def test_draw_interarrival_counters():
    key = ph.replica_key(123, 3)
    # Poisson: one draw
    ia, ctr = ph.draw_interarrival(key, 40, 12.5, "poisson", 0.3)
    assert ctr == 41 and ia == ph.rexp(key, 40, 0.3)
    # off, or rate 0: no draw, never
    assert ph.draw_interarrival(key, 40, 12.5, "off", 6.0) == (ph.D_INF, 40)
    assert ph.draw_interarrival(key, 40, 12.5, "poisson", 0.0) == (ph.D_INF, 40)
    # thinning: two draws per iteration, the accepted gap is the last one
    # proposed, and every earlier proposal was rejected
    seen = set()
    for ctr0 in range(16, 216):
        trace = []
        ia, ctr = ph.draw_interarrival(key, ctr0, 100.0, "sinusoid", 6.0, 0.6,
                                       300.0, trace)
        n_it = len(trace)
        assert ctr == ctr0 + 2 * n_it
        assert ia == ph.rexp(key, ctr0 + 2 * (n_it - 1), R.LAMBD)
        assert all(u > thr for u, thr in trace[:-1])
        assert trace[-1][0] <= trace[-1][1]
        assert trace[-1][0] == ph.philox_u01(key, ctr - 1)
        seen.add(n_it)
    assert {1, 2} <= seen
    # the threshold is the rate at the PROPOSED time t + w, as a share of the
    # envelope
    trace = []
    ph.draw_interarrival(key, 16, 100.0, "sinusoid", 6.0, 0.6, 300.0, trace)
    w = ph.rexp(key, 16, R.LAMBD)
    lam = 6.0 * (1.0 + 0.6 * math.sin(2.0 * math.pi * math.fmod(100.0 + w, 300.0)
                                      / 300.0))
    assert trace[0][1] == lam / R.LAMBD


def _seed_rows(arrivals, seed, total, rank, world):
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.parallel.sharding import replica_shard
    sc = paper_scenario()
    shard = replica_shard(total, rank, world)
    rows = BatchedEngine._seed_arrivals(types.SimpleNamespace(sc=sc),
                                        arrivals[0], arrivals[1], seed, shard)
    return sc, shard, rows


def test_seed_arrivals_use_the_recipes():
    """The host draws stream s's first arrival at counter s under the key of
    the GLOBAL replica id; the kernel then starts at counter n_streams."""
    from distributed_cluster_gpus_amd.configs.paper import build_arrivals
    arrs = build_arrivals()
    sc, shard, rows = _seed_rows(arrs, 123, 24, 2, 3)
    assert (shard.start, shard.count) == (16, 8)
    ns = sc.n_ing * 2
    assert rows.shape == (8, ns)
    for r in range(shard.count):
        key = ph.replica_key(123, 16 + r)
        for s in range(ns):
            if s & 1:      # training: Poisson, one draw at counter s
                assert rows[r, s] == ph.rexp(key, s, arrs[1].rate)
            else:          # inference: thinning at t = 0 on sub-counters
                ia = None
                for sub in range(4096):
                    w = ph.rexp(key, s + ((sub * 2 + 1) << 32), R.LAMBD)
                    lam = 6.0 * (1.0 + 0.6 * math.sin(
                        2.0 * math.pi * math.fmod(w, 300.0) / 300.0))
                    if ph.philox_u01(key, s + ((sub * 2 + 2) << 32)) <= lam / R.LAMBD:
                        ia = w
                        break
                assert rows[r, s] == ia


REPLAY_SEED = 123


@pytest.mark.parametrize("case", ["paper", "poisson", "world3"])
def test_replay_conditions_hold_for_the_chosen_seed(case):
    """test_gpu_rng.py replays these streams against the device; an ulp of
    difference must not be able to reorder two arrivals or flip a thinning
    acceptance."""
    from distributed_cluster_gpus_amd.configs.paper import build_arrivals
    arrs = build_arrivals(inf_mode="poisson") if case == "poisson" \
        else build_arrivals()
    total, rank, world = (24, 2, 3) if case == "world3" else (8, 0, 1)
    sc, shard, rows = _seed_rows(arrs, REPLAY_SEED, total, rank, world)
    for r in range(2):     # the GPU test checks all eight
        rep = R.replay_replica(REPLAY_SEED, shard.start + r, rows[r], arrs,
                               sc.n_dc, 30.0, draws_dc=case != "poisson")
        assert rep.min_gap > 1e-9
        assert rep.min_margin > 1e-12
        assert rep.jid == sum(rep.n_arrivals) == len(rep.jobs) > 500
        per_arrival = 1 if case == "poisson" else 2
        assert rep.ctr >= len(rows[r]) + rep.jid * (per_arrival + 1)
