"""Fused SAC critic-phase kernels (sac_td_target, qr_huber_twin) against
float64 torch.  Tolerances are not fixed numbers: each is 4x the error the
existing torch fp32 path makes against float64 on the same inputs (both are
fp32 evaluations that differ in summation order only)."""
import warnings

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from distributed_cluster_gpus_amd.rl import fused  # noqa: E402
from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,  # noqa: E402
                                                   CHSACAgentConfig)
from distributed_cluster_gpus_amd.rl.sac import quantile_huber_loss  # noqa: E402

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="needs MI355X")


def mod():
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    return load_sim_hip()


def chain(W, s_next, m_dc, m_g, u_dc, u_g, r, done, log_alpha, gamma, dtype,
          force=None):
    """The target chain of rl/sac.py in plain torch at ``dtype``; ``force`` =
    (a_dc, a_g) replaces the argmax.  Returns logits, scores, actions, logp,
    target."""
    W = [w.to(dtype) for w in W]

    def mlp(x, i, n):
        for l in range(i, i + n):
            x = F.linear(x, W[2 * l], W[2 * l + 1])
            x = torch.relu(x) if l < i + n - 1 else x
        return x
    h = torch.relu(mlp(s_next.to(dtype), 0, 3))
    out = {"logits": [], "score": [], "a": [], "lp": 0}
    for k, (i, m, u) in enumerate(((3, m_dc, u_dc), (5, m_g, u_g))):
        logits = mlp(h, i, 2)
        x = logits if m is None else torch.where(
            m, logits, torch.full_like(logits, torch.finfo(torch.float32).min))
        lp_all = torch.log_softmax(x, -1)
        score = lp_all - torch.log(-torch.log(u.to(dtype).clamp_min(1e-20)))
        a = score.argmax(-1) if force is None else force[k]
        out["logits"].append(logits), out["score"].append(score)
        out["a"].append(a)
        out["lp"] = out["lp"] + lp_all.gather(-1, a[:, None])[:, 0]
    x = torch.cat([h] + [F.one_hot(a, w.shape[0]).to(dtype) for a, w in
                         zip(out["a"], (W[8], W[12]))], -1)
    q = torch.min(mlp(x, 7, 3), mlp(x, 10, 3))
    q = q - log_alpha.to(dtype).exp() * out["lp"][:, None]
    out["target"] = r.to(dtype)[:, None] + \
        (1 - done.to(dtype))[:, None] * gamma * q
    return out


def rel_err(x, ref):
    return ((x.double() - ref).abs().max() / (1 + ref.abs().max())).item()


CASES = [(256, 49, 256, 8, 8, 32), (1, 49, 256, 8, 8, 32),
         (17, 3, 256, 8, 8, 32), (17, 49, 32, 3, 5, 8)]


def make_inputs(B, D, H, n_dc, n_g, N, masked, seed=5):
    g = torch.Generator().manual_seed(seed)
    C = H + n_dc + n_g
    shapes = [(H, D), (H, H), (H, H), (H, H), (n_dc, H), (H, H), (n_g, H),
              (H, C), (H, H), (N, H), (H, C), (H, H), (N, H)]
    W = []
    for o, i in shapes:  # nn.Linear's init range
        W += [(torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5,
              (torch.rand(o, generator=g) * 2 - 1) / i ** 0.5]
    s_next = torch.randn(B, D, generator=g) * 50.0
    u_dc, u_g = torch.rand(B, n_dc, generator=g), torch.rand(B, n_g, generator=g)
    m_dc = m_g = None
    if masked:
        m_dc, m_g = (torch.rand(B, n, generator=g) < 0.6 for n in (n_dc, n_g))
        m_dc[0] = False  # one all-false row
    r = torch.randn(B, generator=g)
    done = (torch.arange(B) % 2).float()
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    return ([w.cuda() for w in W], s_next.cuda(), dev(m_dc), dev(m_g),
            u_dc.cuda(), u_g.cuda(), r.cuda(), done.cuda(),
            torch.tensor(-1.3).cuda(), 0.99)


@needs_gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", CASES)
def test_td_target_matches_fp64(shape, masked):
    """Production shape (e32 / kernel, relative to 1 + max|ref|, observed on
    an MI355X): see profiles/README.md, "Fused SAC critic phase"."""
    args = make_inputs(*shape, masked)
    target, a_dc, a_g, logp = mod().sac_td_target(*args)
    ref = chain(*args, torch.float64)
    forced = (a_dc, a_g)
    at64 = chain(*args, torch.float64, force=forced)
    at32 = chain(*args, torch.float32, force=forced)
    # e32: the torch fp32 chain's worst error over logits, logp and target
    e32 = max([rel_err(x, y) for x, y in zip(at32["logits"], ref["logits"])]
              + [rel_err(at32["lp"], at64["lp"]),
                 rel_err(at32["target"], at64["target"])])
    k_lp, k_t = rel_err(logp, at64["lp"]), rel_err(target, at64["target"])
    print(f"{shape} masked={masked}: e32 {e32:.3g}; kernel logp {k_lp:.3g} "
          f"target {k_t:.3g}")
    n_out = 0
    for a, logits, score in zip(forced, ref["logits"], ref["score"]):
        assert a.dtype == torch.int64 and 0 <= a.min() and a.max() < score.shape[1]
        tol = 4 * e32 * (1 + logits.abs().max().item())
        top = score.topk(min(2, score.shape[1]), -1).values
        chosen = score.gather(-1, a[:, None])[:, 0]
        assert (top[:, 0] - chosen).max().item() <= tol
        clear = (top[:, 0] - top[:, -1] > tol) | (score.shape[1] == 1)
        assert torch.equal(a[clear], score.argmax(-1)[clear])
        n_out = max(n_out, int((~clear).sum()))
    assert n_out <= 0.01 * shape[0], f"{n_out} rows inside the score gap"
    assert k_lp <= 4 * e32 and k_t <= 4 * e32, (k_lp, k_t, e32)


@needs_gpu
@pytest.mark.parametrize("B,N", [(1, 32), (5, 8), (256, 32)])
def test_qr_huber_twin_matches_fp64_autograd(B, N):
    g = torch.Generator().manual_seed(B)
    # |pred - target| on both sides of the Huber knee
    q1, q2, tgt = (torch.randn(B, N, generator=g).cuda() * 1.5 for _ in range(3))
    taus = ((torch.arange(N) + 0.5) / N).cuda()
    assert ((q1[:, None] - tgt[:, :, None]).abs() > 1).any()
    assert ((q1[:, None] - tgt[:, :, None]).abs() < 1).any()

    def ref(dtype):
        p1, p2 = (q.to(dtype).clone().requires_grad_() for q in (q1, q2))
        loss = quantile_huber_loss(p1, tgt.to(dtype), taus.to(dtype)) + \
            quantile_huber_loss(p2, tgt.to(dtype), taus.to(dtype))
        return (loss.detach(),) + torch.autograd.grad(loss, (p1, p2))
    r64, r32 = ref(torch.float64), ref(torch.float32)
    got = mod().qr_huber_twin(q1, q2, tgt, taus)
    e32 = max(rel_err(x32, x64) for x32, x64 in zip(r32, r64))
    for name, k, x64 in zip(("loss", "dq1", "dq2"), got, r64):
        ek = rel_err(k, x64)
        print(f"B={B} N={N} {name}: e32 {e32:.3g} kernel {ek:.3g}")
        assert ek <= 4 * e32, (name, ek, e32)
    assert torch.equal(got[0], mod().qr_huber_twin(q1, q2, tgt, taus)[0])
    p1, p2 = q1.clone().requires_grad_(), q2.clone().requires_grad_()
    fused.qr_huber_twin(p1, p2, tgt, taus).backward(torch.tensor(2.0).cuda())
    assert torch.equal(p1.grad, 2 * got[1]) and torch.equal(p2.grad, 2 * got[2])


@needs_gpu
@pytest.mark.parametrize("bad", [dict(H=24), dict(N=65), dict(n_dc=17)])
def test_shape_checks_raise_before_launch(bad):
    dims = dict(B=4, D=9, H=32, n_dc=3, n_g=5, N=8)
    dims.update(bad)
    with pytest.raises(RuntimeError, match="sac_td_target"):
        mod().sac_td_target(*make_inputs(*dims.values(), False))


def paper_agent(fused_critic):
    torch.manual_seed(3)
    return CHSACAgent(CHSACAgentConfig(
        obs_dim=49, n_dc=8, n_g_choices=8, constraints={"latency_p99": 500.0},
        device="cuda", graph_capturable=True, fused_critic=fused_critic))


@needs_gpu
def test_fused_update_matches_eager_and_captures():
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
            agent = paper_agent(on)
            torch.manual_seed(11)
            losses[on] = agent.train_step(batch)["loss_critic"]
    assert agent.algo._fused_ready is True
    # same draws by construction, hence the same actions: the two losses are
    # fp32 evaluations of one O(1) quantity that differ in the targets'
    # summation order.  The pair terms are 1-Lipschitz in the targets, whose
    # fp32 error is a few ulp (2^-23 each) of 1 + max|target|: allow 4 * 2^-20
    # relative to 1 + |loss|, the rule of the kernel tests with e32 = 2^-20.
    assert abs(losses[True] - losses[False]) <= \
        4 * 2.0 ** -20 * (1 + abs(losses[False])), losses
    before = [p.clone() for p in agent.algo.target_critic.parameters()]
    step = GraphedSACStep(agent, ring, 256)
    assert step.captured, step.capture_error
    for _ in range(20):
        step.step()
    torch.cuda.synchronize()
    for m in (agent.encoder, agent.actor, agent.critic, agent.algo.target_critic):
        assert all(torch.isfinite(p).all() for p in m.parameters())
    assert any(not torch.equal(a, b) for a, b in
               zip(before, agent.algo.target_critic.parameters()))
