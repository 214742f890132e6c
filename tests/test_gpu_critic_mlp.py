"""The HIP twin critic (twin_critic_fwd / twin_critic_bwd, rl/fused.py::
twin_critic) against float64 torch.  The bound is the project's rule: 4x the
error the same plain-torch critic makes at float32 against float64 on the same
inputs and ReLU masks (both are fp32 evaluations that differ in summation
order only)."""
import warnings

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from distributed_cluster_gpus_amd.rl import fused  # noqa: E402
from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,  # noqa: E402
                                                   CHSACAgentConfig)
from distributed_cluster_gpus_amd.rl.networks import \
    TwinQuantileCritic  # noqa: E402

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="needs MI355X")

# (B, H, n_dc, n_g, N): production; one row (K = 1 in dW); a row tail with
# N < 16 and C = 39 (unaligned W1 rows); three row tiles, H not a power of
# two, the action and quantile limits
CASES = [(256, 256, 8, 8, 32), (1, 256, 8, 8, 32), (17, 32, 3, 4, 8),
         (33, 48, 16, 16, 64)]
NAMES = ["q1", "q2", "dh"] + [f"d{p}{l}_{c}" for c in "12" for l in "123"
                              for p in "Wb"]
# checked on the CPU: with this seed the torch-fp32 masks stay within the cap
# of mask_exceptions for all four shapes
SEED = 5


def mod():
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    return load_sim_hip()


def make_inputs(B, H, n_dc, n_g, N, device, seed=SEED):
    """A critic with nn.Linear's own init, h = relu(randn), random actions
    and a random upstream gradient."""
    torch.manual_seed(seed)
    critic = TwinQuantileCritic(H, n_dc, n_g, N, hid=H).to(device)
    g = torch.Generator().manual_seed(seed)
    h = torch.relu(torch.randn(B, H, generator=g)).to(device)
    a_dc = torch.randint(0, n_dc, (B,), generator=g).to(device)
    a_g = torch.randint(0, n_g, (B,), generator=g).to(device)
    dq = [torch.randn(B, N, generator=g).to(device) for _ in range(2)]
    return critic, h, a_dc, a_g, dq


def weights(critic):
    return [p.detach() for lin in fused.critic_linears(critic)
            for p in (lin.weight, lin.bias)]


def reference(critic, h, a_dc, a_g, dq, dtype, masks=None):
    """The twin critic in plain torch at ``dtype`` and its gradients under the
    upstream ``dq``.  ``masks[c][l]`` replaces relu(z) by z * mask (None: the
    dtype's own z > 0).  Returns ([q1, q2, dh, 12 grads], [z per (c, l)])."""
    W = [w.to(dtype).clone().requires_grad_() for w in weights(critic)]
    h = h.to(dtype).clone().requires_grad_()
    x = torch.cat([h, F.one_hot(a_dc, critic.n_dc).to(dtype),
                   F.one_hot(a_g, critic.n_g).to(dtype)], -1)
    q, z = [], []
    for c in range(2):
        y = x
        for l in range(2):
            zl = F.linear(y, W[6 * c + 2 * l], W[6 * c + 2 * l + 1])
            m = zl.detach() > 0 if masks is None else masks[c][l]
            y = zl * m.to(dtype)
            z.append(zl.detach())
        q.append(F.linear(y, W[6 * c + 4], W[6 * c + 5]))
    loss = sum((qc * d.to(dtype)).sum() for qc, d in zip(q, dq))
    grads = torch.autograd.grad(loss, [h] + W)
    return [t.detach() for t in q] + list(grads), z


def rel_err(x, ref):
    return ((x.double() - ref).abs().max() / (1 + ref.abs().max())).item()


def mask_exceptions(masks, z64, e32):
    """Hidden units whose mask is not float64's own z64 > 0.  Each must lie
    within the fp32 error of zero; returns how many there are."""
    n = 0
    for k, z in enumerate(z64):
        diff = masks[k // 2][k % 2] != (z > 0)
        assert (z[diff].abs() <= 4 * e32 * (1 + z.abs().max())).all()
        n += int(diff.sum())
    return n


def run(critic, h, a_dc, a_g, dq, weight_grads):
    critic.zero_grad(set_to_none=True)
    hp = h.clone().requires_grad_()
    q1, q2 = fused.twin_critic(critic, hp, a_dc, a_g, weight_grads)
    torch.autograd.backward([q1, q2], dq)
    return [q1.detach(), q2.detach(), hp.grad] + \
        [p.grad for lin in fused.critic_linears(critic)
         for p in (lin.weight, lin.bias)]


@needs_gpu
@pytest.mark.parametrize("shape", CASES)
def test_twin_critic_matches_fp64(shape):
    """Production shape (e32 / kernel, relative to 1 + max|ref|, observed on
    an MI355X): see profiles/README.md, "Fused twin critic"."""
    critic, h, a_dc, a_g, dq = make_inputs(*shape, "cuda")
    act = mod().twin_critic_fwd(weights(critic), h, a_dc, a_g, critic.n_dc,
                                critic.n_g)[2]
    masks = act > 0  # [critic][layer][B][H]: the kernel's own
    r64, z64 = reference(critic, h, a_dc, a_g, dq, torch.float64, masks)
    r32, _ = reference(critic, h, a_dc, a_g, dq, torch.float32, masks)
    e32 = max(rel_err(x, y) for x, y in zip(r32, r64))
    got = run(critic, h, a_dc, a_g, dq, True)
    errs = {n: rel_err(k, ref) for n, k, ref in zip(NAMES, got, r64)}
    print(f"{shape}: e32 {e32:.3g}; kernel max {max(errs.values()):.3g} "
          + " ".join(f"{n} {e:.3g}" for n, e in errs.items()))
    assert max(errs.values()) <= 4 * e32, (errs, e32)
    # at most 1 hidden unit in 10^4 within the fp32 error of zero, none beyond
    n_exc = mask_exceptions(masks, z64, e32)
    print(f"{shape}: {n_exc} of {masks.numel()} masks differ from float64's")
    assert n_exc <= 1e-4 * masks.numel()
    again = run(critic, h, a_dc, a_g, dq, True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    no_w = run(critic, h, a_dc, a_g, dq, False)
    assert all(g is None for g in no_w[3:])
    assert all(torch.equal(a, b) for a, b in zip(got[:3], no_w[:3]))


@needs_gpu
@pytest.mark.parametrize("bad", [dict(H=24), dict(N=65), dict(n_dc=17)])
def test_shape_checks_raise_before_launch(bad):
    dims = dict(B=4, H=32, n_dc=3, n_g=5, N=8)
    dims.update(bad)
    critic, h, a_dc, a_g, _ = make_inputs(*dims.values(), "cuda")
    with pytest.raises(RuntimeError, match="twin_critic"):
        mod().twin_critic_fwd(weights(critic), h, a_dc, a_g, critic.n_dc,
                              critic.n_g)


def paper_agent(fused_critic, fused_critic_mlp):
    torch.manual_seed(3)
    return CHSACAgent(CHSACAgentConfig(
        obs_dim=49, n_dc=8, n_g_choices=8, constraints={"latency_p99": 500.0},
        device="cuda", graph_capturable=True, fused_critic=fused_critic,
        fused_critic_mlp=fused_critic_mlp))


@needs_gpu
def test_mlp_update_matches_eager_and_captures():
    from distributed_cluster_gpus_amd.rl.graphed import GraphedSACStep
    from distributed_cluster_gpus_amd.rl.replay import ReplayRing
    ring = ReplayRing(capacity=1024, obs_dim=49, n_costs=1,
                      cost_names=["latency_p99"], n_dc=8, n_g=8,
                      device="cuda", seed=0)
    torch.manual_seed(1)
    n = 1024
    ring.add_batch(s=torch.randn(n, 49), s_next=torch.randn(n, 49),
                   a_dc=torch.randint(0, 8, (n,)), a_g=torch.randint(0, 8, (n,)),
                   r=torch.randn(n), costs=torch.rand(n, 1) * 100,
                   done=(torch.arange(n) % 2).float())
    batch = ring.sample(256)
    losses = {}
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="fused_critic")  # no fallback
        for on in (False, True):
            agent = paper_agent(False, on)
            torch.manual_seed(11)
            losses[on] = agent.train_step(batch)["loss_critic"]
        assert agent.algo._fused_mlp_ready is True
        # same parameters, draws and targets; q1, q2 are fp32 evaluations that
        # differ in summation order, and the loss is 1-Lipschitz in them: the
        # rule of test_gpu_sac_fused.py with e32 = 2^-20
        assert abs(losses[True] - losses[False]) <= \
            4 * 2.0 ** -20 * (1 + abs(losses[False])), losses
        agent = paper_agent(True, True)
        before = [p.clone() for p in agent.algo.target_critic.parameters()]
        step = GraphedSACStep(agent, ring, 256)
    assert step.captured, step.capture_error
    assert agent.algo._fused_ready and agent.algo._fused_mlp_ready
    for _ in range(20):
        step.step()
    torch.cuda.synchronize()
    for m in (agent.encoder, agent.actor, agent.critic, agent.algo.target_critic):
        assert all(torch.isfinite(p).all() for p in m.parameters())
    assert any(not torch.equal(a, b) for a, b in
               zip(before, agent.algo.target_critic.parameters()))
