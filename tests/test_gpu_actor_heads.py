"""The HIP policy heads (rl/fused.py::actor_heads) against float64 torch: the
actions exactly, the values within 4x the error of the plain-torch fp32 heads
on the same inputs, actions and ReLU masks.  Figures: profiles/README.md."""
import warnings

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from distributed_cluster_gpus_amd.rl import fused  # noqa: E402
from distributed_cluster_gpus_amd.rl.masking import \
    sample_categorical  # noqa: E402
from distributed_cluster_gpus_amd.rl.networks import HybridActor  # noqa: E402
from test_gpu_critic_mlp import mask_exceptions, mod, rel_err  # noqa: E402
from test_gpu_optim_tail import learnables, paper_agent  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X")]

# (B, H, n_dc, n_g): production; one row (K = 1 in dW); a row tail, n < 16, one
# column tile of hidden; three row tiles, H no power of two, the action limit
CASES = [(256, 256, 8, 8), (1, 256, 8, 8), (17, 32, 3, 4), (33, 48, 16, 16)]
NAMES = ["logp", "dh"] + [f"d{p}{l}_{k}" for k in ("dc", "g") for l in "12"
                          for p in "Wb"]
# checked on the CPU with the torch-fp32 heads, all shapes, both mask modes:
# every row passes assert_gap and the ReLU masks pass mask_exceptions' cap
SEED = 5


def single(B):  # rows whose masks allow one action (none when B = 1)
    return [0, B // 2] if B > 1 else []


def make_inputs(B, H, n_dc, n_g, masked, device, seed=SEED):
    """nn.Linear's own init, h = relu(randn).  Masks: the last action masked
    in every row, >= 1 allowed entry per row, exactly one in single(B)'s."""
    torch.manual_seed(seed)
    actor = HybridActor(H, n_dc, n_g, hid=H).to(device)
    g = torch.Generator().manual_seed(seed)
    h = torch.relu(torch.randn(B, H, generator=g))
    u = [torch.rand(B, n, generator=g) for n in (n_dc, n_g)]
    gup = torch.randn(B, generator=g)
    masks = [None, None]
    if masked:
        for k, n in enumerate((n_dc, n_g)):
            m = torch.rand(B, n, generator=g) < 0.6
            keep = torch.randint(0, n - 1, (B,), generator=g)
            m[single(B)] = False
            m[torch.arange(B), keep] = True
            m[:, n - 1] = False
            masks[k] = m.to(device)
    return actor, h.to(device), masks, [x.to(device) for x in u], gup.to(device)


def weights(actor):
    return [p.detach() for lin in fused.head_linears(actor)
            for p in (lin.weight, lin.bias)]


def reference(actor, h, masks, u, gup, dtype, a=None, relu=None):
    """The heads and sample_categorical's arithmetic at ``dtype`` on ``u``;
    ``a[k]`` replaces the dtype's own draw, ``relu[k]`` its own z > 0."""
    W = [w.to(dtype).clone().requires_grad_() for w in weights(actor)]
    h = h.to(dtype).clone().requires_grad_()
    logp, ex = 0, dict(a=[], z=[], lp=[], score=[])
    for k in range(2):
        z = F.linear(h, W[4 * k], W[4 * k + 1])
        m = z.detach() > 0 if relu is None else relu[k]
        x = F.linear(z * m.to(dtype), W[4 * k + 2], W[4 * k + 3])
        if masks[k] is not None:
            x = torch.where(masks[k], x, torch.finfo(dtype).min)
        lp = torch.log_softmax(x, -1)
        uu = u[k].clamp_min(1e-20).to(dtype)
        score = (lp - torch.log(-torch.log(uu))).detach()
        ak = score.argmax(-1) if a is None else a[k]
        logp = logp + lp.gather(-1, ak.unsqueeze(-1)).squeeze(-1)
        for key, v in zip(ex, (ak, z.detach(), lp.detach(), score)):
            ex[key].append(v)
    grads = torch.autograd.grad((logp * gup.to(dtype)).sum(), [h] + W)
    return [logp.detach()] + list(grads), ex


def assert_gap(ex64, ex32, masks):
    """Every row's float64 gap between its two best allowed scores exceeds the
    fp32 error bound on a score: 4 x e32 of lp_all times 1 + max|score|."""
    for k in range(2):
        ok = masks[k] if masks[k] is not None else torch.ones_like(
            ex64["lp"][k], dtype=torch.bool)
        e32 = rel_err(ex32["lp"][k][ok], ex64["lp"][k][ok])
        s = ex64["score"][k].masked_fill(~ok, -float("inf"))
        top = s.topk(2, -1).values
        bound = 4 * e32 * (1 + s[ok].abs().max())
        assert ((top[:, 0] - top[:, 1]) > bound).all(), (k, e32)


def run(actor, h, masks, u, gup, weight_grads):
    actor.zero_grad(set_to_none=True)
    for p in actor.parameters():
        p.requires_grad_(weight_grads)
    hp = h.clone().requires_grad_()
    a_dc, a_g, logp = fused.actor_heads_from_uniforms(actor, hp, *masks, *u)
    logp.backward(gup)
    return [a_dc, a_g, logp.detach(), hp.grad] + \
        [p.grad for lin in fused.head_linears(actor)
         for p in (lin.weight, lin.bias)]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masked"])
@pytest.mark.parametrize("shape", CASES)
def test_actor_heads_match_fp64(shape, masked):
    actor, h, masks, u, gup = make_inputs(*shape, masked, "cuda")
    B, n = shape[0], shape[2:]
    *a, logp2, act, lp_all = mod().actor_heads_fwd(weights(actor), h, *masks,
                                                   *u)
    # actions: exactly float64's, no row excluded
    _, ex64 = reference(actor, h, masks, u, gup, torch.float64)
    _, ex32 = reference(actor, h, masks, u, gup, torch.float32)
    assert_gap(ex64, ex32, masks)
    assert all(torch.equal(x, y) for x, y in zip(a, ex64["a"]))
    # values: float64 at the kernel's own actions and ReLU masks
    relu = act > 0  # [head][B][H]
    r64, _ = reference(actor, h, masks, u, gup, torch.float64, a, relu)
    r32, _ = reference(actor, h, masks, u, gup, torch.float32, a, relu)
    e32 = max(rel_err(x, y) for x, y in zip(r32, r64))
    got = run(actor, h, masks, u, gup, True)
    assert all(torch.equal(x, y) for x, y in zip(got, a))
    assert torch.equal(got[2], logp2[0] + logp2[1])
    errs = {nm: rel_err(x, ref) for nm, x, ref in zip(NAMES, got[2:], r64)}
    # at most 1 hidden unit in 10^4 within the fp32 error of zero, none beyond
    n_exc = mask_exceptions(relu[None], ex64["z"], e32)
    print(f"{shape} masked={masked}: e32 {e32:.3g}; kernel max "
          f"{max(errs.values()):.3g}; {n_exc} masks differ; "
          + " ".join(f"{nm} {e:.3g}" for nm, e in errs.items()))
    assert max(errs.values()) <= 4 * e32, (errs, e32)
    assert n_exc <= 1e-4 * relu.numel()
    if masked:
        dlogits = mod().actor_heads_bwd(weights(actor), h, *a, act, lp_all,
                                        gup, False, False)[2]
        for k, row in [(k, r) for k in range(2) for r in single(B)]:
            # one allowed entry: that action, logp_k = 0, no gradient
            assert masks[k][row].sum() == 1 and masks[k][row, a[k][row]]
            assert logp2[k, row] == 0 and not dlogits[k, row].any()
        for k in range(2):  # masked and padded entries get no gradient
            dW2, db2 = got[4 + 4 * k + 2], got[4 + 4 * k + 3]
            assert not dW2[n[k] - 1].any() and db2[n[k] - 1] == 0
            assert not dlogits[k, :, :n[k]][~masks[k]].any()
            assert not dlogits[k, :, n[k]:].any()
    # a second call has the same bits; detached parameters skip the dW kernel
    again = run(actor, h, masks, u, gup, True)
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    no_w = run(actor, h, masks, u, gup, False)
    assert all(x is None for x in no_w[4:])
    assert all(torch.equal(x, y) for x, y in zip(got[:4], no_w[:4]))


@pytest.mark.parametrize("bad", ["f64 h", "H = 24", "n = 17"])
def test_entry_checks_raise_before_launch(bad):
    dims = dict(B=4, H=24 if bad == "H = 24" else 32,
                n_dc=17 if bad == "n = 17" else 3, n_g=5)
    actor, h, masks, u, _ = make_inputs(*dims.values(), False, "cuda")
    if bad == "f64 h":
        h = h.double()
    with pytest.raises(RuntimeError, match="actor_heads"):
        mod().actor_heads_fwd(weights(actor), h, *masks, *u)


def test_update_matches_torch_path_and_captures():
    from distributed_cluster_gpus_amd.rl.graphed import GraphedSACStep
    from distributed_cluster_gpus_amd.rl.replay import ReplayRing
    ring = ReplayRing(capacity=512, obs_dim=49, n_costs=1, n_dc=8, n_g=8,
                      cost_names=["latency_p99"], device="cuda", seed=0)
    torch.manual_seed(1)
    n = 512
    ring.add_batch(s=torch.randn(n, 49), s_next=torch.randn(n, 49),
                   a_dc=torch.randint(0, 8, (n,)), a_g=torch.randint(0, 8, (n,)),
                   r=torch.randn(n), costs=torch.rand(n, 1) * 100,
                   done=(torch.arange(n) % 2).float(),
                   mask_dc=torch.rand(n, 8) < 0.7, mask_g=torch.rand(n, 8) < 0.7)
    assert ring.mask_dc.any(-1).all() and ring.mask_g.any(-1).all()
    batch = ring.sample(256)
    bm = (batch["mask_dc"], batch["mask_g"])
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="fused_")  # no fallback
        on, off = paper_agent(fused_actor_heads=True), paper_agent()
        # The actor phase's draws under manual_seed(11): the critic phase
        # consumes two [B, 8] uniforms first and leaves encoder and actor as
        # they are.  Same u, fp32 logits that differ in summation order only.
        draws = []
        for agent in (on, off):
            torch.manual_seed(11)
            torch.rand(256, 8, device="cuda"), torch.rand(256, 8, device="cuda")
            with torch.no_grad():
                h = agent.encoder(batch["s"])
                draws.append(
                    fused.actor_heads(agent.actor, h, *bm)[:2] if agent is on
                    else [sample_categorical(x, m)[0]
                          for x, m in zip(agent.actor(h), bm)])
        assert all(torch.equal(x, y) for x, y in zip(*draws))
        for agent in (on, off):
            # as in test_gpu_optim_tail.py, for its reason (slope lr / eps)
            agent.algo.actor_opt.param_groups[0]["eps"] = 1e-4
            torch.manual_seed(11)
            agent.train_step(batch)
        assert on.algo._fused_heads_ready is True
        errs = [rel_err(x, y.double())
                for x, y in zip(learnables(on), learnables(off))]
        print(f"flag on against flag off: {max(errs):.3g} at tensor "
              f"{errs.index(max(errs))}")
        assert len(errs) == 39 and max(errs) <= 4 * 2.0 ** -24, errs
        agent = paper_agent(fused_critic=True, fused_critic_mlp=True,
                            fused_optim=True, fused_actor_heads=True)
        before = [p.clone() for p in learnables(agent)]
        step = GraphedSACStep(agent, ring, 256)
    assert step.captured, step.capture_error
    assert agent.algo._fused_ready and agent.algo._fused_mlp_ready \
        and agent.algo._fused_optim_ready and agent.algo._fused_heads_ready
    for _ in range(5):
        step.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in learnables(agent))
    assert all(not torch.equal(x, y) for x, y in zip(
        before, [*agent.encoder.parameters(), *agent.actor.parameters()]))
