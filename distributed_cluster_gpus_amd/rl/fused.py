"""Fused matrix-core kernels for the SAC critic phase (opt-in).

Two blocks of ``MaskedHybridSAC._critic_phase`` need no autograd graph through
the networks, and each is one HIP kernel (ops/csrc/hip/sac_target.hpp):

* ``sac_td_target`` — encoder(s_next), both actor heads, masked Gumbel-max
  draws, the twin target critic, min, entropy term and the TD line, with the
  activations in LDS from ``s_next`` to the target quantiles;
* ``qr_huber_twin`` — the twin quantile-Huber loss and its closed-form
  gradient in one pass, wrapped here in an autograd Function.

``MaskedHybridSAC(fused_critic=True)`` takes this path when ``unusable``
returns None, and warns once and keeps the torch path otherwise.

``MaskedHybridSAC(fused_critic_mlp=True)`` (independent of the above) also
runs the twin critic itself in HIP (ops/csrc/hip/critic_mlp.hpp):
``twin_critic`` is an autograd Function over a forward kernel that keeps its
activations, a backward kernel for dz and dh, and a weight-gradient kernel
that is launched only when the critic's parameters ask for gradients.

``MaskedHybridSAC(fused_optim=True)`` (independent of both) replaces
``clip_grad_norm_`` + ``Adam.step()`` of each optimizer, and the polyak
average of the target critic, by ``optim_step``: two launches of
ops/csrc/hip/optim_tail.hpp per optimizer, on torch's own Adam state.

``MaskedHybridSAC(fused_actor_heads=True)`` (independent of the three) runs
the two policy heads of the actor phase in HIP (ops/csrc/hip/
actor_heads.hpp): ``actor_heads`` is an autograd Function over a forward
kernel that also draws the masked Gumbel-max actions, a backward kernel that
starts from the closed-form gradient of the chosen log-prob, and a
weight-gradient kernel launched only when a head parameter asks for one.
"""
from typing import List, Optional

import torch
import torch.nn as nn

from .networks import HybridActor, StateEncoder, TwinQuantileCritic

# the kernels' accepted shapes (TORCH_CHECKed again before any launch)
MAX_WIDTH, MAX_ACTIONS, MAX_QUANTILES = 256, 16, 64


def target_linears(algo) -> List[nn.Linear]:
    """The 13 Linear layers of the target chain, in the kernel's order."""
    enc, act, tc = algo.encoder.net, algo.actor, algo.target_critic
    return [enc[0], enc[2], enc[4],
            act.head_dc[0], act.head_dc[2], act.head_g[0], act.head_g[2],
            tc.q1[0], tc.q1[2], tc.q1[4], tc.q2[0], tc.q2[2], tc.q2[4]]


def target_weights(algo) -> List[torch.Tensor]:
    """(weight, bias) of ``target_linears`` — the parameters' own storage, so
    in-place Adam and polyak updates are seen without any copy."""
    out = []
    for lin in target_linears(algo):
        out += [lin.weight.detach(), lin.bias.detach()]
    return out


def critic_linears(critic) -> List[nn.Linear]:
    """The 6 Linear layers of a twin critic, in the kernels' order."""
    return [critic.q1[0], critic.q1[2], critic.q1[4],
            critic.q2[0], critic.q2[2], critic.q2[4]]


def head_linears(actor) -> List[nn.Linear]:
    """The 4 Linear layers of the two policy heads, in the kernels' order."""
    return [actor.head_dc[0], actor.head_dc[2],
            actor.head_g[0], actor.head_g[2]]


def unusable(algo, entry: str = "sac_td_target") -> Optional[str]:
    """Why the fused critic phase cannot serve ``algo`` (None: it can).
    ``entry`` is the extension function the caller needs: the trainable
    critic MLP asks for ``twin_critic_fwd``."""
    if algo.device.type != "cuda":
        return f"the agent is on {algo.device}, not on a GPU"
    if not (type(algo.encoder) is StateEncoder
            and type(algo.actor) is HybridActor
            and type(algo.critic) is TwinQuantileCritic):
        return "the networks are not the standard encoder/actor/critic stacks"
    try:
        shapes = [tuple(lin.weight.shape) for lin in target_linears(algo)]
        typed = all(type(lin) is nn.Linear and lin.bias is not None
                    and lin.weight.dtype == torch.float32
                    for lin in target_linears(algo))
    except (AttributeError, IndexError, TypeError):
        return "the networks are not the standard encoder/actor/critic stacks"
    H, D = shapes[0]
    n_dc, n_g, N = shapes[4][0], shapes[6][0], shapes[9][0]
    C = H + n_dc + n_g
    want = [(H, D), (H, H), (H, H), (H, H), (n_dc, H), (H, H), (n_g, H),
            (H, C), (H, H), (N, H), (H, C), (H, H), (N, H)]
    if not typed or shapes != want:
        return "the layers are not all hid = latent wide f32 Linears"
    if H % 16 or H > MAX_WIDTH or not 1 <= D <= MAX_WIDTH:
        return f"hid = {H} / obs_dim = {D} outside the kernel's range"
    if max(n_dc, n_g) > MAX_ACTIONS or N > MAX_QUANTILES:
        return f"n_dc = {n_dc}, n_g = {n_g}, N = {N} outside the kernel's range"
    try:
        from ..ops import load_sim_hip
        mod = load_sim_hip()
    except ImportError as e:
        return f"the HIP extension does not load ({e})"
    if not hasattr(mod, entry):
        return f"the HIP extension predates the fused critic kernels ({entry})"
    return None


def _mod():
    from ..ops import load_sim_hip
    return load_sim_hip()


@torch.no_grad()
def td_target(algo, s_next, mask_dc, mask_g, r_eff, done, gamma):
    """TD target quantiles [B, N] of one batch.  Draws u_dc then u_g exactly
    as the two ``rand_like`` calls of the torch path do, so both consume the
    device generator alike."""
    B = s_next.shape[0]
    u_dc = torch.rand(B, algo.actor.n_dc, device=s_next.device)
    u_g = torch.rand(B, algo.actor.n_g, device=s_next.device)

    def m(mask):
        return None if mask is None else mask.bool().contiguous()
    target, _, _, _ = _mod().sac_td_target(
        target_weights(algo), s_next.float().contiguous(), m(mask_dc),
        m(mask_g), u_dc, u_g, r_eff.reshape(-1).contiguous(),
        done.reshape(-1).contiguous(), algo.log_alpha.detach(), float(gamma))
    return target


class _QRHuberTwin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q1, q2, target, taus):
        loss, dq1, dq2 = _mod().qr_huber_twin(q1, q2, target, taus)
        ctx.save_for_backward(dq1, dq2)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        dq1, dq2 = ctx.saved_tensors
        return grad_output * dq1, grad_output * dq2, None, None


def qr_huber_twin(q1, q2, target, taus) -> torch.Tensor:
    """quantile_huber_loss(q1, target, taus) + quantile_huber_loss(q2, ...),
    differentiable in q1 and q2."""
    return _QRHuberTwin.apply(q1, q2, target, taus)


class _TwinCritic(torch.autograd.Function):
    """(h, a_dc, a_g, n_dc, n_g, *weights[12]) -> (q1, q2).  The backward
    computes only what autograd asks for: dh if h needs a gradient, the twelve
    weight and bias gradients if any weight does."""

    @staticmethod
    def forward(ctx, h, a_dc, a_g, n_dc, n_g, *weights):
        q1, q2, act = _mod().twin_critic_fwd(list(weights), h, a_dc, a_g,
                                             n_dc, n_g)
        ctx.save_for_backward(h, a_dc, a_g, act, *weights)
        ctx.n = (n_dc, n_g)
        return q1, q2

    @staticmethod
    def backward(ctx, dq1, dq2):
        h, a_dc, a_g, act, *weights = ctx.saved_tensors
        want_dh = ctx.needs_input_grad[0]
        want_dw = any(ctx.needs_input_grad[5:])
        dh, grads = _mod().twin_critic_bwd(
            weights, h, a_dc, a_g, *ctx.n, act, dq1.contiguous(),
            dq2.contiguous(), want_dh, want_dw)
        return (dh, None, None, None, None, *(grads or [None] * 12))


def twin_critic(critic, h, a_dc, a_g, weight_grads: bool):
    """``critic(h, a_dc, a_g)`` on the HIP kernels of ops/csrc/hip/
    critic_mlp.hpp, differentiable in ``h`` and, with ``weight_grads``, in the
    critic's parameters (their gradients reach ``.grad`` by autograd's own
    accumulation).  Without it the weights are passed detached and the
    weight-gradient kernel is not launched."""
    weights = []
    for lin in critic_linears(critic):
        weights += [lin.weight, lin.bias]
    if not weight_grads:
        weights = [w.detach() for w in weights]
    return _TwinCritic.apply(h.float().contiguous(), a_dc.long().contiguous(),
                             a_g.long().contiguous(), critic.n_dc, critic.n_g,
                             *weights)


class _ActorHeads(torch.autograd.Function):
    """(h, mask_dc, mask_g, u_dc, u_g, *weights[8]) -> (a_dc, a_g, logp).  The
    actions carry no gradient.  The backward computes only what autograd asks
    for: dh if h needs a gradient, the eight weight and bias gradients if any
    head parameter does."""

    @staticmethod
    def forward(ctx, h, mask_dc, mask_g, u_dc, u_g, *weights):
        a_dc, a_g, logp2, act, lp_all = _mod().actor_heads_fwd(
            list(weights), h, mask_dc, mask_g, u_dc, u_g)
        ctx.save_for_backward(h, a_dc, a_g, act, lp_all, *weights)
        ctx.mark_non_differentiable(a_dc, a_g)
        return a_dc, a_g, logp2[0] + logp2[1]

    @staticmethod
    def backward(ctx, _da_dc, _da_g, g):
        h, a_dc, a_g, act, lp_all, *weights = ctx.saved_tensors
        want_dh = ctx.needs_input_grad[0]
        want_dw = any(ctx.needs_input_grad[5:])
        dh, grads, _ = _mod().actor_heads_bwd(
            weights, h, a_dc, a_g, act, lp_all, g.contiguous(), want_dh,
            want_dw)
        return (dh, None, None, None, None, *(grads or [None] * 8))


def actor_heads_from_uniforms(actor, h, mask_dc, mask_g, u_dc, u_g):
    """``actor_heads`` on given uniforms ``u_dc [B, n_dc]``, ``u_g [B, n_g]``
    instead of fresh draws from the device generator."""
    def m(mask):
        return None if mask is None else mask.bool().contiguous()
    weights = []
    for lin in head_linears(actor):
        weights += [lin.weight, lin.bias]
    return _ActorHeads.apply(h.float().contiguous(), m(mask_dc), m(mask_g),
                             u_dc, u_g, *weights)


def actor_heads(actor, h, mask_dc, mask_g):
    """``actor(h)`` and the two ``sample_categorical`` draws on the HIP
    kernels of ops/csrc/hip/actor_heads.hpp: returns ``(a_dc, a_g, logp)``
    with ``logp = logp_dc + logp_g`` differentiable in ``h`` and in the eight
    head parameters.  Draws u_dc then u_g exactly as the two ``rand_like``
    calls of the torch path do, so both consume the device generator alike.
    A row whose mask allows no action is not supported."""
    B = h.shape[0]
    u_dc = torch.rand(B, actor.n_dc, device=h.device)
    u_g = torch.rand(B, actor.n_g, device=h.device)
    return actor_heads_from_uniforms(actor, h, mask_dc, mask_g, u_dc, u_g)


# optim_tail's table limit (TORCH_CHECKed again before any launch)
MAX_OPTIM_TENSORS = 32


def optim_unusable(opt) -> Optional[str]:
    """Why ``optim_step`` cannot stand in for ``opt.step()`` (None: it can).
    The kernel bumps Adam's step counters on the device, which only a
    capturable Adam keeps there."""
    if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
        return "the optimizer is not a plain Adam with one param group"
    g = opt.param_groups[0]
    if g["amsgrad"] or g["weight_decay"] != 0 or g["maximize"] \
            or not g["capturable"] or g.get("differentiable") \
            or not isinstance(g["lr"], float):
        return ("Adam is not the default configuration with capturable=True "
                "(amsgrad, weight_decay, maximize, differentiable or a "
                "tensor lr is set)")
    if len(g["params"]) > MAX_OPTIM_TENSORS:
        return f"more than {MAX_OPTIM_TENSORS} tensors in one optimizer"
    if not all(p.dtype == torch.float32 and p.is_contiguous()
               for p in g["params"]):
        return "the parameters are not all contiguous f32"
    return None


@torch.no_grad()
def optim_step(opt, clip_params, max_norm, polyak=None):
    """``clip_grad_norm_(clip_params, max_norm)`` then ``opt.step()`` then,
    with ``polyak=(target_params, tau)`` (paired with the group's parameters
    in order), ``target = (1 - tau) * target + tau * param`` — as one
    ``optim_tail`` call on the optimizer's own Adam state, so checkpoints stay
    interchangeable with the torch path.  A parameter without ``.grad`` is
    skipped as Adam skips it.  ``.grad`` is NOT scaled in place by the clip:
    nothing reads it afterwards, the next ``zero_grad(set_to_none=True)``
    drops it."""
    group = opt.param_groups[0]
    clip_ids = {id(p) for p in clip_params}
    targets, tau = polyak if polyak is not None else (None, 0.0)
    P, G, M, V, S, T, C = [], [], [], [], [], [], []
    for k, p in enumerate(group["params"]):
        if p.grad is None:
            if targets is not None:  # no step, but the target still follows
                targets[k].mul_(1 - tau).add_(tau * p)
            continue
        st = opt.state[p]
        if len(st) == 0:  # as Adam._init_group does for capturable=True
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(
                p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(
                p, memory_format=torch.preserve_format)
        P.append(p)
        G.append(p.grad)
        M.append(st["exp_avg"])
        V.append(st["exp_avg_sq"])
        S.append(st["step"])
        T.append(None if targets is None else targets[k])
        C.append(id(p) in clip_ids)
    if not P:
        return
    beta1, beta2 = group["betas"]
    _mod().optim_tail(P, G, M, V, S, T if targets is not None else [], C,
                      group["lr"], beta1, beta2, group["eps"],
                      float(max_norm), float(tau))
