"""optim_tail (rl/fused.py::optim_step) against float64 torch.  Bound: 4x the
error of the torch path (clip_grad_norm_, Adam(capturable=True), _polyak) at
float32 on the same inputs.  Figures: profiles/README.md, "Fused optimizer"."""
import math
import warnings

import pytest

torch = pytest.importorskip("torch")

from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,  # noqa: E402
                                                   CHSACAgentConfig)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X")]
LR, BETAS, EPS, MAX_NORM, TAU = 1e-2, (0.9, 0.999), 1e-8, 5.0, 0.005
KEYS = ("param", "exp_avg", "exp_avg_sq", "target", "step")


def mod():
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    return load_sim_hip()


def tensor_set(name):
    """[(shape, clipped, has_target, offset)]; offset 1 puts every array of
    the tensor one float into a larger buffer: 4- but not 16-byte aligned."""
    C = mod().optim_tail_chunk
    return {  # the first of "tails" is unclipped like log_alpha
        "tails": [((), False, False, 0), ((1,), True, True, 0),
                  ((3,), True, True, 0), ((5, 7), True, True, 0)],
        "chunks": [((C,), True, True, 0), ((C + 1,), True, True, 0),
                   ((2 * C - 1,), True, True, 0)],
        "table": [((5,), True, k % 2 == 0, 0) for k in range(32)],
        "unaligned": [((C + 3,), True, True, 1), ((6,), True, False, 0)],
    }[name]


def to_gpu(xs, spec):
    return [torch.empty(x.numel() + s[3], device="cuda")[s[3]:].view(x.shape)
            .copy_(x) for x, s in zip(xs, spec)]


def step64(st, grads, spec):
    """One step at float64, in place; returns the clipped tensors' norm."""
    norm = math.sqrt(sum((g * g).sum().item()
                         for g, s in zip(grads, spec) if s[1]))
    coef = min(1.0, MAX_NORM / (norm + 1e-6))
    for k, (_, clipped, has_target, _) in enumerate(spec):
        g = grads[k] * (coef if clipped else 1.0)
        t = st["step"][k].add_(1).item()
        m = st["exp_avg"][k].mul_(BETAS[0]).add_((1 - BETAS[0]) * g)
        v = st["exp_avg_sq"][k].mul_(BETAS[1]).add_((1 - BETAS[1]) * g * g)
        bc1, bc2 = 1 - BETAS[0] ** t, 1 - BETAS[1] ** t
        st["param"][k] -= (LR / bc1) * m / (v.sqrt() / math.sqrt(bc2) + EPS)
        if has_target:
            st["target"][k].mul_(1 - TAU).add_(TAU * st["param"][k])
    return norm


def run_kernel(st, grads, spec):
    targets = [t if s[2] else None for t, s in zip(st["target"], spec)]
    for gs in grads:
        mod().optim_tail(st["param"], to_gpu(gs, spec), st["exp_avg"],
                         st["exp_avg_sq"], st["step"], targets,
                         [s[1] for s in spec], LR, *BETAS, EPS, MAX_NORM, TAU)
    return st


def run_torch(st, grads, spec):
    params = [torch.nn.Parameter(p.clone()) for p in st["param"]]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS,
                           capturable=True)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.cuda()
        torch.nn.utils.clip_grad_norm_(
            [p for p, s in zip(params, spec) if s[1]], MAX_NORM)
        opt.step()
        for p, tp, s in zip(params, st["target"], spec):
            if s[2]:
                tp.mul_(1 - TAU).add_(TAU * p.data)
    return {k: [p.data if k == "param" else opt.state[p][k] for p in params]
            if k != "target" else st[k] for k in KEYS}


def rel_err(x, ref):
    return ((x.double() - ref).abs().max() / (1 + ref.abs().max())).item()


@pytest.mark.parametrize("scale", [3.0, 0.01], ids=["clip", "noclip"])
@pytest.mark.parametrize("name", ["tails", "chunks", "table", "unaligned"])
def test_optim_tail_matches_fp64(name, scale):
    spec = tensor_set(name)
    g = torch.Generator().manual_seed(17)
    st64 = {k: [torch.randn(s[0], generator=g, dtype=torch.float64)
                * (k in ("param", "target")) for s in spec] for k in KEYS[:4]}
    st64["step"] = [torch.zeros((), dtype=torch.float64) for _ in spec]
    grads = [[scale * torch.randn(s[0], generator=g) for s in spec]
             for _ in range(3)]  # three consecutive steps

    def fresh():
        return {k: to_gpu([x.float() for x in st64[k]], spec) for k in KEYS}
    got, again = (run_kernel(fresh(), grads, spec) for _ in range(2))
    t32 = run_torch(fresh(), grads, spec)
    norms = [step64(st64, [x.double() for x in gs], spec) for gs in grads]
    assert all((n > MAX_NORM) == (scale > 1) for n in norms), norms
    e32, err = ({k: max(rel_err(x.cpu(), r) for x, r in zip(res[k], st64[k]))
                 for k in KEYS} for res in (t32, got))
    # floor, where torch is all but exact: one rounding of the largest value
    top = {k: max(r.abs().max().item() for r in st64[k]) for k in KEYS}
    floor = {k: 2.0 ** -24 * top[k] / (1 + top[k]) for k in KEYS}
    print(f"{name} scale {scale}: e32 {max(e32.values()):.3g} kernel "
          f"{max(err.values()):.3g} | " + " ".join(
              f"{k} {e32[k]:.3g}/{err[k]:.3g}" for k in KEYS))
    assert err["step"] == 0 and all(s.item() == 3 for s in got["step"])
    assert all(err[k] <= 4 * max(e32[k], floor[k]) for k in KEYS), (err, e32)
    assert all(torch.equal(a, b) for k in KEYS
               for a, b in zip(got[k], again[k]))


@pytest.mark.parametrize("bad", ["33 tensors", "f64 param", "strided grad",
                                 "i64 step"])
def test_entry_checks_raise_before_launch(bad):
    n = 33 if bad == "33 tensors" else 2
    *lists, steps = ([torch.zeros(4, 6, device="cuda") for _ in range(n)]
                     for _ in range(5))
    steps = [s.sum() for s in steps]
    if bad == "f64 param":
        lists[0][1] = lists[0][1].double()
    if bad == "strided grad":
        lists[1][1] = torch.zeros(6, 4, device="cuda").t()
    if bad == "i64 step":
        steps[1] = steps[1].long()
    with pytest.raises(RuntimeError, match="optim_tail"):
        mod().optim_tail(*lists, steps, [], [True] * n, LR, *BETAS, EPS,
                         MAX_NORM, TAU)
    assert all(not t.any() for l in lists for t in l)


def paper_agent(**flags):
    torch.manual_seed(3)
    return CHSACAgent(CHSACAgentConfig(
        obs_dim=49, n_dc=8, n_g_choices=8, constraints={"latency_p99": 500.0},
        device="cuda", graph_capturable=True, **flags))


def learnables(agent):  # encoder, actor, critic, target critic, log_alpha
    return [p.detach() for p in agent.algo.parameters()] + \
        [agent.algo.log_alpha.detach()]


def test_update_matches_torch_path_captures_and_checkpoints():
    from distributed_cluster_gpus_amd.rl.graphed import GraphedSACStep
    from distributed_cluster_gpus_amd.rl.replay import ReplayRing
    ring = ReplayRing(capacity=512, obs_dim=49, n_costs=1, n_dc=8, n_g=8,
                      cost_names=["latency_p99"], device="cuda", seed=0)
    torch.manual_seed(1)
    n = 512
    ring.add_batch(s=torch.randn(n, 49), s_next=torch.randn(n, 49),
                   a_dc=torch.randint(0, 8, (n,)), a_g=torch.randint(0, 8, (n,)),
                   r=torch.randn(n), costs=torch.rand(n, 1) * 100,
                   done=(torch.arange(n) % 2).float())
    batch = ring.sample(256)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="fused_")  # no fallback
        on, off = paper_agent(fused_optim=True), paper_agent()
        for agent in (on, off):
            # The encoder's gradient passes through the critic just stepped
            # and differs between the agents by that rounding (~1e-9), which
            # Adam's first step lr * g / (|g| + eps) turns into ~1e-6 where
            # |g| ~ eps = 1e-8.  At eps = 1e-4 its slope is <= lr / eps = 3.
            agent.algo.actor_opt.param_groups[0]["eps"] = 1e-4
            torch.manual_seed(11)
            agent.train_step(batch)
        assert on.algo._fused_optim_ready is True
        # test 1's rule with e32 = 2^-24, float32's unit roundoff, half the
        # smallest e32 that test 1 measures
        errs = [rel_err(a, b.double())
                for a, b in zip(learnables(on), learnables(off))]
        print(f"flag on against flag off: {max(errs):.3g}")
        assert len(errs) == 39 and max(errs) <= 4 * 2.0 ** -24, errs

        layout = [(sd["param_groups"], [
            (k, f, v.dtype, v.shape, v.device) for k, st in sd["state"].items()
            for f, v in st.items()]) for sd in (on.algo.critic_opt.state_dict(),
                                                off.algo.critic_opt.state_dict())]
        assert layout[0] == layout[1]
        # a checkpoint of the flag-on agent trains on in a flag-off agent
        off.load_state_dict(on.state_dict())
        assert all(torch.equal(a, b)
                   for a, b in zip(learnables(on), learnables(off)))
        assert all(math.isfinite(v) for v in off.train_step(batch).values())
        agent = paper_agent(fused_critic=True, fused_critic_mlp=True,
                            fused_optim=True)
        before = [p.clone() for p in agent.algo.target_critic.parameters()]
        step = GraphedSACStep(agent, ring, 256)
    assert step.captured, step.capture_error
    assert agent.algo._fused_ready and agent.algo._fused_mlp_ready \
        and agent.algo._fused_optim_ready
    for _ in range(20):
        step.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in learnables(agent))
    assert any(not torch.equal(a, b) for a, b in
               zip(before, agent.algo.target_critic.parameters()))
