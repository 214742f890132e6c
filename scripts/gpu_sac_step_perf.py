"""Graph-replayed SAC step rate with the fused critic phase off ("off"), on
("on") and on together with the HIP twin critic ("mlp": fused_critic +
fused_critic_mlp) and with the fused optimizer tail on top ("opt": mlp +
fused_optim) and the HIP policy heads on top of that ("heads": opt +
fused_actor_heads), and the isolated time of each fused kernel against the
torch code it replaces.

Same agent, ring and batch as bench.py::measure_rl_steps_per_sec.  All
steppers live in one process and are timed in alternation (--repeats windows
of --steps replays each, after --warmup replays), so drift on a shared host
hits all alike; the spread printed is min..max over the windows.

    python scripts/gpu_sac_step_perf.py [--steps 300] [--repeats 7]

Prints one JSON line.  For per-step kernel counts run it once per mode under
``rocprofv3 --kernel-trace --stats -- python scripts/gpu_sac_step_perf.py
--only off|on|mlp|opt|heads --repeats 1`` and divide the call counts by the replays."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from distributed_cluster_gpus_amd.rl import fused  # noqa: E402
from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,  # noqa: E402
                                                   CHSACAgentConfig)
from distributed_cluster_gpus_amd.rl.graphed import GraphedSACStep  # noqa: E402
from distributed_cluster_gpus_amd.rl.replay import ReplayRing  # noqa: E402
from distributed_cluster_gpus_amd.rl.sac import quantile_huber_loss  # noqa: E402

OBS, BATCH = 49, 256
MODES = ("off", "on", "mlp", "opt", "heads")


def make_stepper(fused_critic, fused_critic_mlp=False, fused_optim=False,
                 fused_actor_heads=False):
    torch.manual_seed(0)
    agent = CHSACAgent(CHSACAgentConfig(
        obs_dim=OBS, n_dc=8, n_g_choices=8,
        constraints={"latency_p99": 500.0, "gpu_over": 0.0}, device="cuda",
        graph_capturable=True, fused_critic=fused_critic,
        fused_critic_mlp=fused_critic_mlp, fused_optim=fused_optim,
        fused_actor_heads=fused_actor_heads))
    ring = ReplayRing(capacity=4096, obs_dim=OBS, n_costs=2,
                      cost_names=["latency_p99", "gpu_over"], n_dc=8, n_g=8,
                      device="cuda", seed=0)
    B = 4096
    ring.add_batch(s=torch.randn(B, OBS), s_next=torch.randn(B, OBS),
                   a_dc=torch.randint(0, 8, (B,)), a_g=torch.randint(0, 8, (B,)),
                   r=torch.randn(B), costs=torch.rand(B, 2) * 100,
                   done=torch.ones(B))
    step = GraphedSACStep(agent, ring, BATCH)
    if not step.captured:
        raise RuntimeError(f"capture failed: {step.capture_error}")
    if fused_critic and not agent.algo._fused_ready:
        raise RuntimeError("the fused critic phase fell back to torch")
    if fused_critic_mlp and not agent.algo._fused_mlp_ready:
        raise RuntimeError("the HIP twin critic fell back to torch")
    if fused_optim and not agent.algo._fused_optim_ready:
        raise RuntimeError("the fused optimizer tail fell back to torch")
    if fused_actor_heads and not agent.algo._fused_heads_ready:
        raise RuntimeError("the HIP policy heads fell back to torch")
    return step


def window(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step.step()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def event_us(fn, iters=200, warmup=20):
    for _ in range(warmup):
        fn()
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def isolated(algo):
    """Eager per-call time (launch overhead included on both sides) of each
    block at B = 256: the fused kernel and the torch code it replaces."""
    dev = algo.device
    s_next = torch.randn(BATCH, OBS, device=dev)
    mask = torch.ones(BATCH, 8, dtype=torch.bool, device=dev)
    r, done = torch.randn(BATCH, 1, device=dev), torch.zeros(BATCH, 1, device=dev)
    q1, q2, tgt = (torch.randn(BATCH, 32, device=dev) for _ in range(3))
    q1.requires_grad_(), q2.requires_grad_()

    @torch.no_grad()
    def torch_target():
        h = algo.encoder(s_next)
        q, _ = algo._target_quantiles(h, mask, mask)
        return r + (1 - done) * 0.99 * q

    def torch_loss():
        loss = quantile_huber_loss(q1, tgt, algo.taus) + \
            quantile_huber_loss(q2, tgt, algo.taus)
        return torch.autograd.grad(loss, (q1, q2))

    def fused_loss():
        return torch.autograd.grad(fused.qr_huber_twin(q1, q2, tgt, algo.taus),
                                   (q1, q2))
    return {
        "td_target_torch_us": event_us(torch_target),
        "td_target_fused_us": event_us(
            lambda: fused.td_target(algo, s_next, mask, mask, r, done, 0.99)),
        "qr_huber_torch_us": event_us(torch_loss),
        "qr_huber_fused_us": event_us(fused_loss),
    }


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--only", default=None,
                   help="comma-separated subset of off,on,mlp,opt,heads")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    only = args.only.split(",") if args.only else MODES
    if not set(only) <= set(MODES):
        raise SystemExit(f"--only takes a subset of {','.join(MODES)}")
    modes = [m for m in MODES if m in only]
    steppers = {m: make_stepper(m != "off", m in ("mlp", "opt", "heads"),
                                m in ("opt", "heads"), m == "heads")
                for m in modes}
    for s in steppers.values():
        window(s, args.warmup)
    rates = {m: [] for m in modes}
    for _ in range(args.repeats):
        for m in modes:  # alternate
            rates[m].append(window(steppers[m], args.steps))
    out = {"batch": BATCH, "steps_per_window": args.steps,
           "repeats": args.repeats}
    for m in modes:
        out[f"steps_per_s_{m}"] = {
            "median": round(statistics.median(rates[m]), 1),
            "min": round(min(rates[m]), 1), "max": round(max(rates[m]), 1)}
    if args.only is None:
        out["speedup_median"] = round(out["steps_per_s_on"]["median"] /
                                      out["steps_per_s_off"]["median"], 3)
        out["speedup_mlp_over_on_median"] = round(
            out["steps_per_s_mlp"]["median"] /
            out["steps_per_s_on"]["median"], 3)
    if "mlp" in modes and "opt" in modes:
        out["speedup_opt_over_mlp_median"] = round(
            out["steps_per_s_opt"]["median"] /
            out["steps_per_s_mlp"]["median"], 3)
    if "opt" in modes and "heads" in modes:
        out["speedup_heads_over_opt_median"] = round(
            out["steps_per_s_heads"]["median"] /
            out["steps_per_s_opt"]["median"], 3)
    if args.only is None:
        out.update({k: round(v, 1) for k, v in
                    isolated(steppers["on"].agent.algo).items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
