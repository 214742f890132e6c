#!/usr/bin/env python3
"""Cost of arrival mode 'profile' on the GPU: the bench.py step loop (paper
topology, default_policy) under two workloads, alternating in one process:
the default one (inference a sinusoid, thinned: two draws per round) and its
profile-mode twin, ``ArrivalProcess.diurnal(rate, amp, period, zero offsets,
segments=24)`` (exact inversion: one draw per arrival).  The two are different
arrival processes, so the outputs differ; what is compared is events/s.

Events/s per round, the median and the max - min spread, for each replica
count.  With ``--once`` the script runs each workload's step loop once and
nothing else: the form to run under ``rocprofv3 --kernel-trace --stats`` for
the two generators' kernel times.

Usage: gpu_profile_perf.py [--once] [rounds [steps [events_per_step
                           [replicas ...]]]]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_cluster_gpus_amd.configs.paper import build_arrivals, paper_scenario
from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess

WORKLOADS = ("sinusoid", "profile")


def arrivals(workload):
    inf, trn = build_arrivals()
    if workload == "profile":
        inf = ArrivalProcess.diurnal(inf.rate, inf.amp, inf.period,
                                     [0.0] * paper_scenario().n_ing,
                                     segments=24)
    return inf, trn


def step_loop(replicas, workload, steps, warmup=3, events_per_step=4000):
    """events/s of `steps` advance calls after `warmup`, as bench.py times
    them."""
    duration = max(1200.0, (warmup + steps) * events_per_step / 100.0)
    inf, trn = arrivals(workload)
    eng = BatchedEngine(paper_scenario(), inf, trn, algo="default_policy",
                        replicas=replicas, duration=duration, log_interval=5.0,
                        out_dir=None, seed=123,
                        # bench.py's rule: 65k replicas fit one GPU at 8192
                        qcap=int(max(24576 if replicas <= 16384 else 8192,
                                     8 * duration)), enable_logs=False)
    assert ("arr_prof" in eng.t) == (workload == "profile")
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
    jobs = float(eng.t["jid_ctr"].double().mean().item())
    return (int(ev.sum().item()) - ev0) / wall, jobs


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] +
                                                       xs[len(xs) // 2])


if __name__ == "__main__":
    argv = sys.argv[1:]
    once = "--once" in argv
    a = [int(x) for x in argv if x != "--once"]
    rounds, steps, eps = (a[:3] + [5, 10, 4000][len(a[:3]):])
    sizes = a[3:] or [4096, 65536]
    for replicas in sizes:
        rates = {w: [] for w in WORKLOADS}
        for rnd in range(1 if once else rounds):
            for w in WORKLOADS:
                torch.cuda.empty_cache()
                rate, jobs = step_loop(replicas, w, steps, events_per_step=eps)
                rates[w].append(rate)
                print(json.dumps({"workload": w, "round": rnd,
                                  "replicas": replicas, "steps": steps,
                                  "events_per_sec": round(rate),
                                  "arrivals_per_replica": round(jobs, 1)}),
                      flush=True)
        if once:
            continue
        out = {"replicas": replicas, "rounds": rounds}
        for w in WORKLOADS:
            out[w + "_median"] = round(median(rates[w]))
            out[w + "_spread"] = round(max(rates[w]) - min(rates[w]))
        out["profile_minus_sinusoid"] = out["profile_median"] - \
            out["sinusoid_median"]
        print(json.dumps(out), flush=True)
