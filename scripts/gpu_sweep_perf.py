#!/usr/bin/env python3
"""Cost of a parameter sweep on the GPU: the bench.py step loop (paper
topology) for default_policy and cap_greedy, the plain engine against an
all-base sweep of 8 groups (identical work, identical outputs: the difference
is the feature's overhead), alternating in one process; then one real sweep,
8 load points x 512 replicas, for the events/s a user sees.

The claim under test: the sweep engine's median is not below the plain
engine's by more than the plain engine's own max - min spread over the rounds.

Usage: gpu_sweep_perf.py [replicas [rounds [steps [events_per_step]]]]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_cluster_gpus_amd.configs.paper import build_arrivals, paper_scenario
from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
from distributed_cluster_gpus_amd.engine.sweep import Sweep

GROUPS = 8
CAP_W = 45000.0   # between the 30 and 60 kW the tests use as active caps


def step_loop(replicas, algo, sweep, steps, warmup=3, events_per_step=4000):
    """events/s of `steps` advance calls after `warmup`, as bench.py times
    them."""
    duration = max(1200.0, (warmup + steps) * events_per_step / 100.0)
    sc = paper_scenario()
    inf, trn = build_arrivals()
    eng = BatchedEngine(sc, inf, trn, algo=algo, replicas=replicas,
                        duration=duration, log_interval=5.0, out_dir=None,
                        seed=123, qcap=int(max(24576, 8 * duration)),
                        power_cap=CAP_W if algo == "cap_greedy" else 0.0,
                        enable_logs=False, sweep=sweep)
    ev = eng.t["ev_count"]
    for _ in range(warmup):
        eng._sim.advance(duration, events_per_step)
    torch.cuda.synchronize()
    ev0 = int(ev.sum().item())
    t0 = time.perf_counter()
    for _ in range(steps):
        eng._sim.advance(duration, events_per_step)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert int(eng.t["err"].max().item()) == 0
    assert int(eng.t["done"].max().item()) == 0, "a replica finished"
    return (int(ev.sum().item()) - ev0) / wall, eng


def all_base(algo):
    """8 groups, every point the base: through the swept-cap kernel for
    cap_greedy, through the sweep generator for both"""
    if algo == "cap_greedy":
        return Sweep.grid(power_cap=[CAP_W] * GROUPS)
    return Sweep.grid(inf_rate=[build_arrivals()[0].rate] * GROUPS)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] +
                                                       xs[len(xs) // 2])


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    replicas, rounds, steps, eps = (a + [4096, 5, 10, 4000][len(a):])[:4]
    for algo in ("default_policy", "cap_greedy"):
        rates = {False: [], True: []}
        last = {}
        for rnd in range(rounds):
            for swept in (False, True):
                torch.cuda.empty_cache()
                rate, eng = step_loop(replicas, algo,
                                      all_base(algo) if swept else None,
                                      steps, events_per_step=eps)
                rates[swept].append(rate)
                last[swept] = {k: eng.t[k].clone() for k in
                               ("ev_count", "energy_j", "jobs_done", "now")}
                del eng
                print(json.dumps({"algo": algo, "round": rnd, "sweep": swept,
                                  "replicas": replicas, "steps": steps,
                                  "events_per_sec": round(rate)}), flush=True)
        same = all(torch.equal(last[False][k], last[True][k])
                   for k in last[False])
        spread = max(rates[False]) - min(rates[False])
        m_plain, m_sweep = median(rates[False]), median(rates[True])
        print(json.dumps({
            "algo": algo, "rounds": rounds, "outputs_equal": same,
            "plain_median": round(m_plain), "sweep_median": round(m_sweep),
            "plain_spread": round(spread),
            "sweep_minus_plain": round(m_sweep - m_plain),
            "within_spread": bool(m_sweep >= m_plain - spread)}), flush=True)
    # one real sweep: 8 load points x 512 replicas
    loads = [2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]
    torch.cuda.empty_cache()
    rate, eng = step_loop(len(loads) * 512, "default_policy",
                          Sweep.grid(inf_rate=loads), steps,
                          events_per_step=eps)
    st = eng.sweep_stats()
    print(json.dumps({"real_sweep": {"inf_rate": loads, "replicas": eng.R,
                                     "events_per_sec": round(rate),
                                     "jobs_mean_per_group":
                                     [round(x, 1) for x in st.mean[:, 1]]}}),
          flush=True)
