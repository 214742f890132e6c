"""engine/state.py on the CPU: the placeholders and initial contents of the
allocation, the config dict, and the strict checkpoint load."""
import numpy as np
import pytest
import torch

from distributed_cluster_gpus_amd.configs.paper import build_arrivals
from distributed_cluster_gpus_amd.engine.state import (INF, P99_WIN,
                                                       alloc_state,
                                                       engine_cfg,
                                                       engine_dims,
                                                       load_tensors,
                                                       policy_weights_numel)

R, TCAP, QCAP, TR_CAP = 3, 8, 16, 32


def _state(sc, algo, **kw):
    trace = kw.pop("arrival_trace", None)
    dims = engine_dims(sc, algo=algo, n_rep=R, tcap=TCAP, qcap=QCAP,
                       tr_cap=TR_CAP, arrival_trace=trace, **kw)
    return dims, alloc_state(dims, sc, "cpu", trace)


def test_placeholders_follow_the_configuration(paper_sc):
    sc = paper_sc
    TS, D, F = int(sc.total_gpus.sum()), sc.n_dc, sc.n_freq
    _, t = _state(sc, "default_policy")
    assert t["snap_f"].shape == (1, 1)
    assert t["b_n"].shape == t["b_s"].shape == (1, D, 2, F)
    assert "p99_sorted" not in t and "req_flag" not in t
    _, t = _state(sc, "cap_greedy")
    assert t["snap_f"].shape == (R, TS) and t["b_n"].shape == (1, D, 2, F)
    _, t = _state(sc, "bandit")
    assert t["snap_f"].shape == (1, 1)
    assert t["b_n"].shape == t["b_s"].shape == (R, D, 2, F)
    _, t = _state(sc, "chsac_af")
    assert t["p99_sorted"].shape == t["p99_ring"].shape == (1, 1, 1)
    assert t["policy_weights"].shape == (1,)
    _, t = _state(sc, "chsac_af", rl_exact_p99=True, serve_device=True)
    assert t["p99_sorted"].shape == t["p99_ring"].shape == (R, 2, P99_WIN)
    assert t["policy_weights"].numel() == policy_weights_numel(
        1 + 6 * D, D, int(sc.policy.max_gpus_per_job))
    _, t = _state(sc, "chsac_af", weights_buffer=True)
    assert t["policy_weights"].numel() > 1


def test_initial_contents(paper_sc):
    sc = paper_sc
    dims, t = _state(sc, "default_policy", log_interval=5.0)
    NS = sc.n_ing * 2
    assert t["rng_ctr"].dtype == torch.int64 and (t["rng_ctr"] == NS).all()
    assert (t["arr_next"] == INF).all() and t["arr_next"].shape == (R, NS)
    assert (t["now"] == -1.0).all() and (t["next_log"] == 5.0).all()
    assert (t["s_finish"] == INF).all() and (t["x_time"] == INF).all()
    assert (t["dc_min_finish"] == INF).all() and (t["dc_min_slot"] == -1).all()
    assert (t["util_begin"] == -1.0).all()
    assert torch.equal(t["cur_freq"], torch.as_tensor(
        sc.default_freq, dtype=torch.float64).expand(R, -1))
    off = t["slot_off"].numpy()
    assert off[0] == 0 and (np.diff(off) == sc.total_gpus).all()
    assert (np.bincount(t["slot_dc"].numpy()) == sc.total_gpus).all()
    assert t["s_rec"].shape == (R, dims.total_slots, 8)
    assert t["x_rec"].shape == (R, TCAP, 4)
    assert all(v.is_contiguous() and v.device.type == "cpu"
               for v in t.values())
    # logs off: single-row buffers; on: sized from the run
    assert t["cl_rows"].shape == (1, 15) and t["jl_rows"].shape == (1, 11)
    dims, t = _state(sc, "default_policy", log_replica=0, duration=100.0,
                     log_interval=10.0, events_per_launch=50000)
    assert t["cl_rows"].shape == (sc.n_dc * 12 + 64, 15)
    assert t["jl_rows"].shape == (100000, 11)


def test_trace_mode_seeds_arrivals_from_the_trace(paper_sc):
    sc = paper_sc
    NS = sc.n_ing * 2
    tt = np.cumsum(np.random.default_rng(0).random((R, NS, 4)), axis=2)
    dims, t = _state(sc, "default_policy", arrival_trace=(tt, tt * 2))
    assert dims.trace_mode and dims.trace_cap == 4
    assert torch.equal(t["arr_next"], torch.as_tensor(tt[:, :, 0]))
    assert (t["trace_dc"] == -1).all() and t["trace_dc"].dtype == torch.int8
    assert t["trace_pos"].shape == (R, NS)
    cfg = engine_cfg(dims, sc, *build_arrivals())
    assert cfg["trace_mode"] == 1 and cfg["trace_cap"] == 4


def test_cfg_carries_every_option_without_fallbacks(paper_sc):
    sc = paper_sc
    inf, trn = build_arrivals()
    dims, _ = _state(sc, "default_policy", pop_series_every=3,
                     duration=100.0, log_interval=10.0)
    cfg = engine_cfg(dims, sc, inf, trn)
    assert cfg["algo"] == 0 and cfg["tr_cap"] == 0 and cfg["pp_cap"] == 0
    assert cfg["serve_device"] == 0 and cfg["exact_p99"] == 0
    assert cfg["tr_limit"] == 0 and cfg["elastic"] == 0 and cfg["rl_det"] == 0
    assert cfg["pop_series_every"] == 3 and dims.ps_cap == 10 // 3 + 2
    assert cfg["obs_dim"] == 1 + 6 * sc.n_dc and cfg["p99_win"] == P99_WIN
    dims, _ = _state(sc, "chsac_af", elastic_scaling=True, serve_device=True,
                     rl_deterministic=True, rl_train_interval=4)
    cfg = engine_cfg(dims, sc, inf, trn)
    assert cfg["algo"] == 8 and cfg["tr_cap"] == TR_CAP
    assert cfg["pp_cap"] == int(sc.total_gpus.max())
    assert cfg["elastic"] == 1 and cfg["serve_device"] == 1
    assert cfg["rl_det"] == 1 and cfg["tr_limit"] == min(TR_CAP // 2, 4 * 256)
    # elastic scaling is a chsac feature
    dims, _ = _state(sc, "joint_nf", elastic_scaling=True)
    assert engine_cfg(dims, sc, inf, trn)["elastic"] == 0


# ---- load_state's strict copy ------------------------------------------
def _saved(t):
    return {k: v.clone() for k, v in t.items()}


def test_load_rejects_a_placeholder_against_a_full_tensor(paper_sc):
    _, full = _state(paper_sc, "cap_greedy")
    _, other = _state(paper_sc, "default_policy")
    saved = _saved(full)
    saved["snap_f"] = other["snap_f"]          # (1, 1): copy_ would broadcast
    saved["snap_f"].fill_(7.0)
    with pytest.raises(ValueError, match="'snap_f'.*\\(1, 1\\)"):
        load_tensors(full, saved)
    assert (full["snap_f"] == 0).all()         # nothing was copied


def test_load_rejects_missing_extra_and_retyped_keys(paper_sc):
    _, t = _state(paper_sc, "default_policy")
    saved = _saved(t)
    del saved["q_len"]
    saved["now"].fill_(3.0)
    with pytest.raises(ValueError, match="lacks tensor 'q_len'"):
        load_tensors(t, saved)
    assert (t["now"] == -1.0).all()
    saved = _saved(t)
    saved["ps_tick"] = torch.zeros(R, dtype=torch.int32)
    with pytest.raises(ValueError, match="'ps_tick' is not part"):
        load_tensors(t, saved)
    saved = _saved(t)
    saved["busy"] = saved["busy"].to(torch.int64)
    with pytest.raises(ValueError, match="'busy'.*int64.*int32"):
        load_tensors(t, saved)


def test_load_copies_an_exact_match(paper_sc):
    _, t = _state(paper_sc, "chsac_af", rl_exact_p99=True)
    saved = _saved(t)
    for k, v in saved.items():
        v.copy_(torch.arange(v.numel()).reshape(v.shape) % 100)
    load_tensors(t, saved)
    assert all(torch.equal(t[k], saved[k]) for k in t)
    assert set(t) == set(saved)


def test_cpu_state_does_not_alias_the_scenario():
    """torch.as_tensor shares memory with a numpy array on the CPU; writing
    the state (a run, a checkpoint load) must not write the scenario."""
    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    sc = paper_scenario()
    want = sc.total_gpus.copy(), np.array(sc.freq_levels, copy=True)
    _, t = _state(sc, "default_policy")
    for v in t.values():
        v.zero_()
    assert (sc.total_gpus == want[0]).all()
    assert (np.asarray(sc.freq_levels) == want[1]).all()
