#!/usr/bin/env python3
"""Cost of the per-replica latency histograms on the GPU: the bench.py step
loop (default_policy, paper topology) with latency_hist off and on,
alternating in one process, and the time of one latency_reduce over the
histograms of the last recording run.

Usage: gpu_latency_hist_perf.py [replicas [rounds [steps [events_per_step]]]]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_cluster_gpus_amd.configs.paper import build_arrivals, paper_scenario
from distributed_cluster_gpus_amd.engine.batched import BatchedEngine


def step_loop(replicas, on, steps, warmup=3, events_per_step=4000):
    """events/s of `steps` advance calls after `warmup`, as bench.py times
    them; returns the engine too."""
    duration = max(1200.0, (warmup + steps) * events_per_step / 100.0)
    sc = paper_scenario()
    inf, trn = build_arrivals()
    eng = BatchedEngine(sc, inf, trn, algo="default_policy",
                        replicas=replicas, duration=duration,
                        log_interval=5.0, out_dir=None, seed=123,
                        qcap=int(max(24576, 8 * duration)),
                        enable_logs=False, latency_hist=on)
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


def time_reduce(eng, calls=20, warmup=5):
    """Device-event times (ms) of latency_reduce on the engine's histograms."""
    lh = eng.latency_hist()
    qs = torch.tensor([0.5, 0.9, 0.99, 0.999], dtype=torch.float64)
    ms = []
    for i in range(warmup + calls):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        eng._mod.latency_reduce(lh["hist"], lh["over"], qs)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4),
            "max_ms": round(ms[-1], 4)}


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    replicas, rounds, steps, eps = (a + [4096, 4, 10, 4000][len(a):])[:4]
    eng = None
    for rnd in range(rounds):
        for on in (False, True):
            del eng
            torch.cuda.empty_cache()
            rate, eng = step_loop(replicas, on, steps, events_per_step=eps)
            print(json.dumps({"round": rnd, "latency_hist": on,
                              "replicas": replicas, "steps": steps,
                              "events_per_sec": round(rate)}), flush=True)
    jobs = int(eng.t["lh_hist"].sum().item())
    print(json.dumps({"latency_reduce": time_reduce(eng), "replicas": replicas,
                      "jobs_in_hist": jobs,
                      "hist_mib": round(eng.t["lh_hist"].numel() * 4 / 2**20, 1)}),
          flush=True)
