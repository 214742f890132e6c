"""GPU tests for the 64-lane engine's event-select path: the DPP wave
reductions, the ballot first-empty-slot search and the conditional min-finish
rescan.

Three layers:
  1. the production reduction helpers, driven row by row through the
     extension's debug entry points, against numpy (value by bit pattern,
     lane / index exactly);
  2. the 64-lane engine against the 8-lane engine, which keeps the
     __shfl_xor butterflies and the per-lane slot search and so is an
     independent implementation of the same reductions: every tensor
     bench.py dumps must be torch.equal;
  3. the cached per-DC min finish (value and slot) recomputed on the host
     from s_finish after a congested run, unsplit and split into many short
     launches.

The engine comparisons of layer 2 were first run on the commit before the DPP
reductions: default_policy, the congested debug configuration, joint_nf,
eco_route, bandit and cap_greedy (60 kW cap) were all already identical
between the two builds there, so all four algorithms of case (c) stay in the
parametrisation.
"""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="needs MI355X")

INF = 1e300
INT_MAX = 2**31 - 1


def _mod():
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    return load_sim_hip("_sim_hip")


# ---------------------------------------------------------------- layer 1

def _reduction_rows():
    """(vals[B,64] f64, idx[B,64] i32): the edge cases first, then random
    rows up to 256.  Index rows are permutations (or all INT_MAX next to an
    all-sentinel row, as the engine's empty candidates are), so the expected
    winner is always unique."""
    rng = np.random.default_rng(7)
    ident = np.arange(64, dtype=np.int32)
    rev = ident[::-1].copy()
    vals, idx = [], []

    def add(v, i):
        vals.append(np.asarray(v, dtype=np.float64).copy())
        idx.append(np.asarray(i, dtype=np.int32).copy())

    def shuffled():
        return rng.permutation(64).astype(np.int32)

    sent = np.full(64, INF)
    # all sentinel
    add(sent, ident)
    add(sent, np.full(64, INT_MAX, dtype=np.int32))
    add(sent, shuffled())
    # a single finite value at the row / half-wave boundaries
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):
        v = sent.copy()
        v[lane] = 12.5 + lane
        add(v, ident)
        add(v, shuffled())
    # duplicated minimum across the DPP stage boundaries
    for a, b in ((15, 16), (31, 32), (0, 63), (47, 48)):
        v = 100.0 + rng.random(64)
        v[a] = v[b] = 3.25
        add(v, ident)
        add(v, rev)           # the higher lane holds the lower index
        add(v, shuffled())    # non-monotonic indices
        v2 = sent.copy()
        v2[a] = v2[b] = 3.25
        add(v2, shuffled())
    # +0.0 against -0.0: equal under ==, different bit patterns
    for a, b in ((3, 40), (15, 16), (31, 32), (0, 63)):
        for za, zb in ((0.0, -0.0), (-0.0, 0.0)):
            v = 1.0 + rng.random(64)
            v[a], v[b] = za, zb
            add(v, ident)
            add(v, rev)
            add(v, shuffled())
    # negative values
    for _ in range(8):
        add(-1e6 * rng.random(64) - 1.0, shuffled())
    v = sent.copy()
    v[20], v[52] = -7.0, -7.0
    add(v, rev)
    # random rows: continuous, and small-integer rows full of ties
    while len(vals) < 256:
        if len(vals) % 2:
            add(rng.normal(size=64) * 1e3, shuffled())
        else:
            add(rng.integers(0, 4, size=64).astype(np.float64), shuffled())
    return np.stack(vals), np.stack(idx)


def _expected_reductions(vals, idx):
    B = vals.shape[0]
    v_lane = np.empty(B)
    o_lane = np.empty(B, dtype=np.int32)
    v_idx = np.empty(B)
    o_idx = np.empty(B, dtype=np.int32)
    for r in range(B):
        row, ix = vals[r], idx[r]
        tied = np.flatnonzero(row == row.min())   # == : +0.0 ties -0.0
        lane = tied.min()                         # lowest absolute lane
        v_lane[r], o_lane[r] = row[lane], lane
        w = tied[np.argmin(ix[tied])]             # lowest candidate index
        v_idx[r], o_idx[r] = row[w], ix[w]
    return v_lane, o_lane, v_idx, o_idx


@needs_gpu
def test_wave_argmin_helpers_match_numpy():
    vals, idx = _reduction_rows()
    assert vals.shape == (256, 64)
    out = _mod().wave_reduce_debug(torch.from_numpy(vals).cuda(),
                                   torch.from_numpy(idx).cuda())
    g_vl, g_l, g_vi, g_i = (o.cpu().numpy() for o in out)
    e_vl, e_l, e_vi, e_i = _expected_reductions(vals, idx)
    assert np.array_equal(g_l, e_l), np.flatnonzero(g_l != e_l)
    assert np.array_equal(g_vl.view(np.int64), e_vl.view(np.int64))
    assert np.array_equal(g_i, e_i), np.flatnonzero(g_i != e_i)
    assert np.array_equal(g_vi.view(np.int64), e_vi.view(np.int64))


@needs_gpu
def test_first_empty_matches_numpy():
    def run(rows):
        got = _mod().first_empty_debug(torch.from_numpy(rows).cuda())
        exp = np.array([np.flatnonzero(r >= INF)[0] if (r >= INF).any()
                        else INT_MAX for r in rows], dtype=np.int32)
        assert np.array_equal(got.cpu().numpy(), exp), (got, exp)
        return exp

    rng = np.random.default_rng(3)
    # one full chunk, nothing empty -> sentinel
    full64 = 1.0 + rng.random((2, 64))
    assert (run(full64) == INT_MAX).all()
    one = full64.copy()
    one[0, 63] = INF
    one[1, 0] = INF
    run(one)
    # three chunks, the last partial
    L = 186
    rows = 1.0 + rng.random((6, L))
    rows[0, 0] = INF                       # index 0 only
    rows[1, 64] = INF                      # first lane of the second chunk
    rows[2, L - 1] = INF                   # last element of the partial chunk
    rows[3, [70, 71, 130, L - 1]] = INF    # several: lowest wins
    rows[4, [185, 128, 127]] = np.inf      # several, +inf counts as empty
    exp = run(rows)                        # rows[5]: none empty
    assert list(exp) == [0, 64, L - 1, 70, 127, INT_MAX]


# ---------------------------------------------------------------- layer 2

def _engine(case, subwave, **over):
    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    kw = dict(replicas=16, duration=60.0, log_interval=5.0, out_dir=None,
              enable_logs=False, subwave=subwave)
    if case == "congested":
        # the configuration of test_queueing_delay_metric_positive_under_
        # congestion: saturated DCs, so finishes drain queues; tcap=256
        inf = ArrivalProcess(mode="poisson", rate=30.0)
        trn = ArrivalProcess(mode="poisson", rate=2.0)
        kw.update(algo="debug", seed=11, num_fixed_gpus=8, fixed_freq=0.3,
                  tcap=256)
    else:
        inf, trn = build_arrivals()
        kw.update(algo=case, seed=123)
        if case == "cap_greedy":
            kw.update(power_cap=60000.0)
    kw.update(over)
    eng = BatchedEngine(sc, inf, trn, **kw)
    st = eng.run()
    assert st["events"] > 0 and int(eng.t["err"].max().item()) == 0
    return eng, st


@functools.lru_cache(maxsize=None)
def _run64(case):
    return _engine(case, 64)


CASES = ["default_policy", "congested",
         "joint_nf", "eco_route", "bandit", "cap_greedy"]


@needs_gpu
@pytest.mark.parametrize("case", CASES)
def test_64_lane_engine_equals_8_lane_engine(case):
    sys.path.insert(0, REPO)
    from bench import DUMP_TENSORS
    e64, st64 = _run64(case)
    e8, _ = _engine(case, 8)
    if case == "congested":
        assert st64["mean_wait_s"] > 0.0, "the congested case never queued"
    for name in DUMP_TENSORS:
        assert torch.equal(e64.t[name].cpu(), e8.t[name].cpu()), name


# ---------------------------------------------------------------- layer 3

def _check_min_finish_cache(eng):
    assert eng.validate_state()
    t = eng.t
    fin = t["s_finish"].cpu()                       # [R, slots]
    slot_dc = t["slot_dc"].cpu().long()             # [slots]
    minf = t["dc_min_finish"].cpu().reshape(fin.shape[0], -1)
    mins = t["dc_min_slot"].cpu().reshape(fin.shape[0], -1).long()
    n_dc = minf.shape[1]
    busy_dcs = 0
    for d in range(n_dc):
        cols = torch.nonzero(slot_dc == d).flatten()
        ref = fin[:, cols].min(dim=1).values.clamp(max=INF)
        assert torch.equal(minf[:, d], ref), f"dc {d}: cached min finish"
        has = ref < INF
        busy_dcs += int(has.sum())
        assert bool((mins[~has, d] == -1).all()), f"dc {d}: slot of empty DC"
        s = mins[has, d]
        assert bool((slot_dc[s] == d).all()), f"dc {d}: slot outside the DC"
        assert torch.equal(fin[has].gather(1, s[:, None])[:, 0], ref[has]), \
            f"dc {d}: cached slot does not hold the min"
    assert busy_dcs > 0, "nothing running at the end: the check is vacuous"


@needs_gpu
def test_min_finish_cache_exact_after_congested_run():
    eng, _ = _run64("congested")
    _check_min_finish_cache(eng)


@needs_gpu
def test_min_finish_cache_exact_across_short_launches():
    eng, _ = _engine("congested", 64, events_per_launch=500)
    _check_min_finish_cache(eng)
