"""engine/rl_loop.py on the CPU: the train pacer against the three formulas it
replaced, the serving weight buffer's layout, mask expansion, and the
synchronous cycle (serve / ingest / train) over CPU tensors and a stub sim."""
import pytest
import torch

from distributed_cluster_gpus_amd.engine.rl_loop import (RLDriver,
                                                         ServingWeights,
                                                         expand_mask,
                                                         make_learner,
                                                         pace_train)
from distributed_cluster_gpus_amd.engine.state import (RL_HID, alloc_state,
                                                       engine_dims,
                                                       policy_weights_numel)
from distributed_cluster_gpus_amd.rl.agent import CHSACAgentConfig, make_agent

OBS, N_DC, N_G = 49, 8, 8


# ---------------- pacer ----------------
# The three places the rule was written out before it became pace_train,
# copied literally (self._x -> plain names).
def _formula_dp(backlog, tr_total, min_replay, warmup, batch, interval, world):
    backlog += tr_total
    steps = 0
    if min_replay >= max(warmup, batch):
        per_step = interval * world
        steps = min(64, backlog // per_step)
        backlog -= steps * per_step
    return steps, backlog


def _formula_single(backlog, n_new, replay_size, warmup, batch, interval, world):
    backlog += n_new
    steps = 0
    if replay_size >= warmup:
        steps = min(64, backlog // interval)
        backlog -= steps * interval
    return steps, backlog


def _formula_rl_service(backlog, n_new, replay_size, warmup, batch, interval,
                        world):
    backlog = backlog + n_new
    steps = 0
    if replay_size >= warmup:
        steps = min(64, backlog // interval)
        backlog -= steps * interval
    return steps, backlog


# (n_new, replay_size) per launch: below the gate (backlog accumulates),
# crossing warmup=100 and then batch=200, a backlog worth more than 64 steps
# (capped, remainder carried over several launches), then a trickle
SEQ = [(10, 10), (30, 40), (50, 90), (25, 115), (60, 175), (40, 215),
       (5000, 5215), (0, 5215), (0, 5215), (0, 5215), (7, 5222), (41, 5263)]


@pytest.mark.parametrize("formula,world,warmup,batch", [
    (_formula_single, 1, 100, 32),
    (_formula_rl_service, 1, 100, 32),
    (_formula_dp, 2, 100, 32),
    (_formula_dp, 1, 100, 32),
    (_formula_single, 1, 100, 200),   # batch > warmup, single-rank gate
    (_formula_dp, 2, 100, 200),       # batch > warmup, data-parallel gate
])
def test_pacer_matches_the_formulas_it_replaced(formula, world, warmup, batch):
    interval = 16
    gate = max(warmup, batch) if formula is _formula_dp else warmup
    backlog = ref_backlog = 0
    trace = []
    for n_new, replay_size in SEQ:
        steps, backlog = pace_train(backlog, n_new, replay_size, interval,
                                    world if formula is _formula_dp else 1,
                                    gate)
        ref_steps, ref_backlog = formula(ref_backlog, n_new, replay_size,
                                         warmup, batch, interval, world)
        assert (steps, backlog) == (ref_steps, ref_backlog)
        trace.append(steps)
    assert trace[0] == 0 and max(trace) == 64   # gated, then capped
    assert trace.count(64) >= 2                 # the remainder was carried


def test_pacer_gates_differ_when_batch_exceeds_warmup():
    """warmup 100 < batch 200, replay at 115: a single rank trains, data-
    parallel ranks do not — as before; which is right is an open question."""
    single = pace_train(90, 25, 115, 16, 1, gate=100)
    dp = pace_train(90, 25, 115, 16, 1, gate=max(100, 200))
    assert single == (7, 3) and dp == (0, 115)


# ---------------- serving weight buffer ----------------
def _agent(**kw):
    return make_agent(CHSACAgentConfig(
        obs_dim=OBS, n_dc=N_DC, n_g_choices=N_G,
        constraints={"latency_p99": 500.0, "gpu_over": 0.0}, device="cpu",
        **kw))


def _layer_slices(agent):
    """Expected buffer content, layer by layer, in the documented order."""
    enc, act = agent.encoder.net, agent.actor
    lins = [enc[0], enc[2], enc[4], act.head_dc[0], act.head_dc[2],
            act.head_g[0], act.head_g[2]]
    return [torch.cat([l.weight.detach().t().contiguous().flatten(),
                       l.bias.detach()]) for l in lins]


def test_weight_buffer_layout_and_refresh():
    torch.manual_seed(0)
    agent = _agent()
    assert ServingWeights.servable(agent, OBS, N_DC, N_G, RL_HID)
    buf = torch.zeros(policy_weights_numel(OBS, N_DC, N_G, RL_HID))
    w = ServingWeights(agent, buf, OBS, N_DC, N_G, RL_HID)
    assert sum(dst.numel() for dst, _ in w.pairs) == buf.numel()
    w.refresh()
    want = _layer_slices(agent)
    assert torch.equal(buf, torch.cat(want))
    # change one parameter in place: only its slice moves
    before = buf.clone()
    with torch.no_grad():
        agent.actor.head_dc[2].bias.add_(1.0)
    w.refresh()
    want = _layer_slices(agent)
    assert torch.equal(buf, torch.cat(want))
    off = sum(s.numel() for s in want[:4]) + N_DC * RL_HID
    changed = (buf != before).nonzero().flatten()
    assert changed.tolist() == list(range(off, off + N_DC))


def test_agents_that_are_not_servable():
    class NoEncoderNet:
        encoder = object()
    for agent in (_agent(latent_dim=128), NoEncoderNet()):
        assert not ServingWeights.servable(agent, OBS, N_DC, N_G, RL_HID)
    with pytest.raises(ValueError):
        ServingWeights(_agent(latent_dim=128), torch.zeros(8), OBS, N_DC, N_G,
                       RL_HID)


# ---------------- mask expansion ----------------
def test_expand_mask():
    m = expand_mask(torch.tensor([0, 1, 0x80, 0xFF], dtype=torch.uint8), 8)
    assert m.dtype == torch.bool
    assert m.tolist() == [[False] * 8,
                          [True] + [False] * 7,
                          [False] * 7 + [True],
                          [True] * 8]
    m = expand_mask(torch.tensor([0x05], dtype=torch.int32), 3)
    assert m.tolist() == [[True, False, True]]


# ---------------- synchronous cycle ----------------
R, TR_CAP = 4, 32
TIMING_KEYS = ("advance_s", "serve_s", "dp_sync_s", "train_s",
               "overlap_train_steps", "launches", "sync0_s", "kernel_s",
               "status_s", "ingest_s", "floor_s", "refresh_s")
REQ_FLAG = [1, 0, 1, 2]     # pending, idle, pending, already answered
REQ_MDC = [0x04, 0xFF, 0x00, 0xFF]   # replica 0: DC 2 only; replica 2: none
REQ_MG = [0x10, 0xFF, 0x0F, 0xFF]    # replica 0: g 4 only; replica 2: g 0..3
UNTOUCHED = -7


class StubSim:
    """advance() leaves what a launch would: parked requests and `n_tr`
    transition rows, from a script with one entry per launch."""

    def __init__(self, t, script):
        self.t, self.script, self.launches = t, script, 0

    def advance(self, end_time, events):
        t, (n_tr, err) = self.t, self.script[self.launches]
        self.launches += 1
        g = torch.Generator().manual_seed(self.launches)
        t["req_flag"].copy_(torch.tensor(REQ_FLAG))
        t["req_obs"].copy_(torch.randn(R, OBS, generator=g))
        t["req_mdc"].copy_(torch.tensor(REQ_MDC))
        t["req_mg"].copy_(torch.tensor(REQ_MG))
        t["resp_dc"].fill_(UNTOUCHED)
        t["resp_g"].fill_(UNTOUCHED)
        for k in ("tr_s0", "tr_s1", "tr_r", "tr_costs"):
            t[k][:n_tr] = torch.randn(t[k][:n_tr].shape, generator=g)
        for k, hi in (("tr_adc", N_DC), ("tr_ag", N_G), ("tr_mdc", 256),
                      ("tr_mg", 256)):
            t[k][:n_tr] = torch.randint(0, hi, (n_tr,), generator=g)
        t["tr_count"].fill_(n_tr)
        t["err"][1] = err


def _driver(paper_sc, script, deterministic=False):
    torch.manual_seed(0)
    dims = engine_dims(paper_sc, algo="chsac_af", n_rep=R, tcap=8, qcap=16,
                       tr_cap=TR_CAP)
    assert (dims.obs_dim, paper_sc.n_dc) == (OBS, N_DC)
    t = alloc_state(dims, paper_sc, "cpu")
    agent, replay = make_learner(OBS, N_DC, N_G, "cpu", world=1, seed=0,
                                 buffer=64, sla_p99_ms=500.0, agent=_agent())
    drv = RLDriver(t, StubSim(t, script), None, torch.device("cpu"),
                   agent=agent, replay=replay, obs_dim=OBS, n_dc=N_DC,
                   n_g=N_G, hid=RL_HID, serve_device=False, mfma_serve=False,
                   deterministic=deterministic, batch=4, warmup=4,
                   train_interval=2, stats_interval=0, end_time=1.0,
                   events_per_launch=1, drain_job_rows=lambda n_jl: None)
    tm = dict.fromkeys(TIMING_KEYS, 0.0)
    tm["launches"] = 0
    cycle = drv.start_run(tm)
    assert cycle == drv.cycle_sync
    return drv, cycle, tm


@pytest.mark.parametrize("deterministic", [False, True])
def test_sync_cycle_serves_only_pending_replicas_within_masks(paper_sc,
                                                              deterministic):
    drv, cycle, _ = _driver(paper_sc, [(0, 0)], deterministic)
    seen = {}
    inner = drv.rl.select_action_batch

    def spy(obs, m_dc, m_g, deterministic=False):
        seen["m_dc"], seen["m_g"] = m_dc.clone(), m_g.clone()
        return inner(obs, m_dc, m_g, deterministic=deterministic)

    drv.rl.select_action_batch = spy
    assert cycle() is False
    t = drv.t
    assert t["req_flag"].tolist() == [2, 0, 2, 2]
    dc, g = t["resp_dc"].tolist(), t["resp_g"].tolist()
    assert (dc[1], g[1], dc[3], g[3]) == (UNTOUCHED,) * 4
    if deterministic:
        # parity mode answers with the scalar entry's greedy action, one
        # request at a time (the greedy head does not consult the masks)
        for r in (0, 2):
            a = drv.rl.select_action(t["req_obs"][r].numpy(), None, None,
                                     deterministic=True)
            assert (dc[r], g[r]) == (a["dc"], a["g"])
        assert "m_dc" not in seen
    else:
        assert (dc[0], g[0]) == (2, 4)       # the only choices its masks allow
        assert 0 <= dc[2] < N_DC and 0 <= g[2] < 4   # all-zero DC mask opened
        assert seen["m_dc"].tolist() == [[i == 2 for i in range(N_DC)],
                                         [True] * N_DC]
        assert seen["m_g"].tolist() == [[i == 4 for i in range(N_G)],
                                        [i < 4 for i in range(N_G)]]


def test_sync_cycle_ingests_and_trains_at_the_pacers_count(paper_sc):
    script = [(3, 0), (5, 0), (1, 0), (6, 0)]
    drv, cycle, tm = _driver(paper_sc, script)
    calls = {"n": 0}
    inner = drv.rl.train_step

    def counting(batch, compute_stats=True):
        calls["n"] += 1
        return inner(batch, compute_stats=compute_stats)

    drv.rl.train_step = counting
    t, rp = drv.t, drv.replay
    backlog, per_cycle = 0, []
    for n_tr, _ in script:
        size0, calls0, upd0 = rp.size, calls["n"], drv.rl_updates
        cycle()
        rows = slice(size0, size0 + n_tr)
        assert rp.size == size0 + n_tr
        assert torch.equal(rp.s[rows], t["tr_s0"][:n_tr])
        assert torch.equal(rp.s_next[rows], t["tr_s1"][:n_tr])
        assert torch.equal(rp.a_dc[rows], t["tr_adc"][:n_tr].long())
        assert torch.equal(rp.a_g[rows], t["tr_ag"][:n_tr].long())
        assert torch.equal(rp.r[rows], t["tr_r"][:n_tr])
        assert torch.equal(rp.costs[rows], t["tr_costs"][:n_tr])
        assert torch.equal(rp.done[rows], torch.ones(n_tr))
        assert torch.equal(rp.mask_dc[rows],
                           expand_mask(t["tr_mdc"][:n_tr], N_DC))
        assert torch.equal(rp.mask_g[rows], expand_mask(t["tr_mg"][:n_tr], N_G))
        assert int(t["tr_count"]) == 0
        steps, backlog = pace_train(backlog, n_tr, rp.size, 2, 1, gate=4)
        assert calls["n"] - calls0 == drv.rl_updates - upd0 == steps
        per_cycle.append(steps)
    assert per_cycle == [0, 4, 0, 3] and drv.backlog == backlog == 1
    assert tm["launches"] == len(script)


def test_sync_cycle_raises_on_error_flags_before_serving(paper_sc):
    drv, cycle, _ = _driver(paper_sc, [(5, 0x4)])
    with pytest.raises(RuntimeError, match="error flags: 0x4 "):
        cycle()
    t = drv.t
    assert t["req_flag"].tolist() == REQ_FLAG
    assert t["resp_dc"].tolist() == [UNTOUCHED] * R
    assert drv.replay.size == 0 and int(t["tr_count"]) == 5
