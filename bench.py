#!/usr/bin/env python3
"""Flagship benchmark: batched Monte-Carlo replica engine on the paper
multi-DC config (BASELINE.json metric: simulated events/sec, whole node).

One step = every replica advancing by `--events-per-step` simulation events
through the gfx950 advance kernel.  Weak scaling: each GPU owns
`--replicas-per-gpu` replicas, so per-GPU work is fixed as N grows; the
reported value is the WHOLE-JOB aggregate events/sec over all ranks.

Launch (driver contract):
  python bench.py --gpus N --steps K --warmup W
  # N>1: torchrun --nnodes=1 --nproc-per-node N bench.py --gpus N ...

Reference baseline: 4,003 events/sec — the pure-Python
reference simulator, default_policy, paper topology, sinusoid inference
arrivals 6/s amp 0.6 period 300 + poisson training 0.3/s, measured on one
CPU core.  Same algorithm, same topology, same arrival processes here.

A plain run sets up, warms up, times the steps and prints the result line.
`--dump-outputs DIR` also writes the per-replica state left by the last timed
step as DIR/<name>.npy; with the same arguments the inputs (Philox streams
keyed on seed and replica id) are identical from run to run, so two builds
can be compared array for array.

`--full` adds the secondary RL metrics (CHSAC-AF SAC updates/sec on-device,
batch 256 — BASELINE.md: 36.9/s on CPU — and RL-in-the-loop events/sec),
measured OUTSIDE the timed region and reported inside config; without it
those config fields are null.
"""
import argparse
import json
import os
import time


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--replicas-per-gpu", type=int, default=4096)
    p.add_argument("--events-per-step", type=int, default=4000)
    p.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                   help="weak: each GPU owns --replicas-per-gpu replicas "
                        "(per-GPU work fixed); strong: --replicas-per-gpu is "
                        "the FIXED GLOBAL replica pool, sharded over ranks")
    p.add_argument("--algo", type=str, default="default_policy")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--subwave", type=int, default=64, choices=[8, 64])
    p.add_argument("--fp32-coeff", type=int, default=0,
                   help="opt-in fp32 decision-score eval in the sim kernels")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the secondary "
                        "measurements (CHSAC-AF SAC updates/sec and "
                        "RL-in-the-loop throughput); a plain run skips them")
    p.add_argument("--with-rl", type=int, default=1,
                   help="with --full: measure the CHSAC-AF metrics (untimed "
                        "region); 0 leaves them out")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="write the per-replica state the timed path produced "
                        "in its last step as DIR/<name>.npy (float64)")
    args = p.parse_args(argv)
    if args.steps < 1:
        p.error("--steps must be at least 1")
    if args.warmup < 0:
        p.error("--warmup must not be negative")
    return args


# Per-replica tensors the advance kernel hands back to a caller (the inputs
# of BatchedEngine.stats() / metrics_tensors() plus the simulation clocks and
# per-DC occupancy).  Replica-major, a few hundred KB at the default size.
DUMP_TENSORS = ("now", "ev_count", "jobs_done", "jobs_done_inf", "sum_lat",
                "sum_lat_inf", "sum_wait", "energy_j", "util_time", "busy",
                "cur_freq", "n_running", "p_active", "jid_ctr", "rng_ctr")


def dump_outputs(eng, out_dir, rank, world):
    """Write the engine's per-replica outputs as float64 .npy files.  Counters
    stay far below 2**53, so the conversion is exact.  With several ranks
    each writes its own shard as <name>_rank<r>.npy."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if world == 1 else f"_rank{rank}"
    for name in DUMP_TENSORS:
        arr = eng.t[name].detach().cpu().numpy().astype(np.float64)
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), arr)


def measure_rl_steps_per_sec(device, n_updates=200, batch=256):
    """CHSAC-AF train-step rate on the paper obs space (49-dim, 8 DC, 8 g),
    using the production path: hipGraph-captured step when available
    (rl/graphed.py), eager otherwise."""
    import torch

    from distributed_cluster_gpus_amd.rl.agent import CHSACAgent, CHSACAgentConfig
    from distributed_cluster_gpus_amd.rl.graphed import GraphedSACStep
    from distributed_cluster_gpus_amd.rl.replay import ReplayRing
    torch.manual_seed(0)
    obs_dim = 49
    on_gpu = device.type == "cuda"
    agent = CHSACAgent(CHSACAgentConfig(
        obs_dim=obs_dim, n_dc=8, n_g_choices=8,
        constraints={"latency_p99": 500.0, "gpu_over": 0.0},
        device=str(device), graph_capturable=on_gpu))
    ring = ReplayRing(capacity=4096, obs_dim=obs_dim, n_costs=2,
                      cost_names=["latency_p99", "gpu_over"], n_dc=8, n_g=8,
                      device=str(device), seed=0)
    B = 4096
    ring.add_batch(s=torch.randn(B, obs_dim), s_next=torch.randn(B, obs_dim),
                   a_dc=torch.randint(0, 8, (B,)), a_g=torch.randint(0, 8, (B,)),
                   r=torch.randn(B), costs=torch.rand(B, 2) * 100,
                   done=torch.ones(B))
    stepper = None
    if on_gpu:
        stepper = GraphedSACStep(agent, ring, batch)
        if not stepper.captured:
            stepper = None

    def one_step():
        if stepper is not None:
            stepper.step()
        else:
            agent.train_step(ring.sample(batch), compute_stats=False)

    for _ in range(10):  # warmup
        one_step()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_updates):
        one_step()
    if on_gpu:
        torch.cuda.synchronize()
    return n_updates / (time.perf_counter() - t0)


def measure_rl_loop(device, wall_budget_s=8.0, replicas=4096):
    """CHSAC-AF RL-IN-THE-LOOP throughput (BASELINE config 4's shape): the
    batched engine with in-kernel policy serving, transitions streaming into
    replay and SAC training at the production cadence.  Reference baseline:
    127 events/s (BASELINE.md chsac_af run).  Untimed region of the bench."""
    import time as _t

    import torch

    from distributed_cluster_gpus_amd.configs.paper import paper_scenario
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    sc = paper_scenario()
    inf = ArrivalProcess(mode="sinusoid", rate=6.0, amp=0.6, period=300.0)
    trn = ArrivalProcess(mode="poisson", rate=0.3)
    eng = BatchedEngine(sc, inf, trn, algo="chsac_af", replicas=replicas,
                        duration=1e9, log_interval=20.0, out_dir=None,
                        seed=1, enable_logs=False, rl_warmup=2048,
                        rl_batch=256, rl_train_interval=256,
                        rl_stats_interval=0, events_per_launch=100000)
    # warm phase: fill replay past warmup, capture the train graph, settle
    # clocks — then time the production overlapped loop itself
    eng.run(max_wall_s=3.0)
    torch.cuda.synchronize(device)
    ev0 = int(eng.t["ev_count"].sum().item())
    up0 = eng.rl_updates
    t0 = _t.perf_counter()
    eng.run(max_wall_s=wall_budget_s)
    torch.cuda.synchronize(device)
    el = _t.perf_counter() - t0
    return ((int(eng.t["ev_count"].sum().item()) - ev0) / el,
            (eng.rl_updates - up0) / el)


def main():
    args = parse_args()
    import torch

    from distributed_cluster_gpus_amd.configs.paper import (build_arrivals,
                                                            paper_scenario)
    from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
    from distributed_cluster_gpus_amd.parallel.dist import (allreduce_scalar,
                                                            barrier,
                                                            init_distributed,
                                                            is_distributed)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        init_distributed("nccl")
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    if not torch.cuda.is_available():
        raise RuntimeError("bench.py requires a ROCm GPU")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)

    total_replicas = (args.replicas_per_gpu * world if args.scaling == "weak"
                      else args.replicas_per_gpu)
    total_steps = args.warmup + args.steps
    # duration generous enough that no replica reaches end_time mid-bench
    # (~150-200 events per simulated second per replica on this workload)
    duration = max(1200.0, total_steps * args.events_per_step / 100.0)
    # queue capacity: generous default; at huge replica counts the per-entry
    # f64 pair (size + enqueue time) dominates HBM, so scale it down — paper
    # workload queues stay in the hundreds (288 GB sizing note)
    qcap = int(max(24576 if total_replicas <= 16384 else 8192, 8 * duration))

    if args.algo == "chsac_af":
        raise SystemExit("chsac_af is measured by the RL-in-the-loop metric "
                         "(rl_loop_events_per_sec, reported with --full);"
                         " the raw step loop would bypass training/ingest")
    sc = paper_scenario()
    inf, trn = build_arrivals()  # sinusoid 6/s amp .6 period 300; poisson 0.3/s
    eng = BatchedEngine(sc, inf, trn, algo=args.algo,
                        replicas=total_replicas, duration=duration,
                        log_interval=5.0, out_dir=None, seed=args.seed,
                        device=device, rank=rank, world=world, qcap=qcap,
                        enable_logs=False, subwave=args.subwave,
                        fp32_coeff_eval=bool(args.fp32_coeff))

    ev = eng.t["ev_count"]

    def step():
        eng._sim.advance(duration, args.events_per_step)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(device)
    ev_start = int(ev.sum().item())

    barrier()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(device)
    barrier()
    t1 = time.perf_counter()

    if int(eng.t["err"].max().item()) != 0:
        raise RuntimeError("engine error flags set during bench")
    if int(eng.t["done"].max().item()) != 0:
        raise RuntimeError("a replica finished inside the timed region; "
                           "raise --events-per-step headroom (invalid run)")

    elapsed = t1 - t0
    events = float(int(ev.sum().item()) - ev_start)
    # whole-job aggregate: sum events over ranks; MAX elapsed over ranks
    if is_distributed():
        events = allreduce_scalar(events, device=device)
        import torch.distributed as dist
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    value = events / elapsed

    if args.dump_outputs:
        dump_outputs(eng, args.dump_outputs, rank, world)

    rl_steps_s = None
    rl_loop_ev_s = rl_loop_up_s = None
    if args.full and args.with_rl and rank == 0:
        rl_steps_s = measure_rl_steps_per_sec(device)
        rl_loop_ev_s, rl_loop_up_s = measure_rl_loop(device)

    if rank == 0:
        baseline = 4003.0  # BASELINE.md reference events/sec (CPU, 1 core)
        out = {
            "metric": "sim_events_per_sec",
            "value": value,
            "unit": "events/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": value / baseline,
            "dtype": "fp64",
            "data": "synthetic",
            "config": {
                "model": "paper_config multi-DC geo-cluster DES",
                "global_batch": total_replicas,
                "seq_len": args.events_per_step,
                "parallelism": f"replica_shard_dp{world}",
                "algo": args.algo,
                "replicas_per_gpu": total_replicas // world,
                "events_per_step": args.events_per_step,
                "arrivals": "sinusoid inf 6/s amp 0.6 period 300 + poisson trn 0.3/s",
                "fp32_coeff_eval": bool(args.fp32_coeff),
                "topology": "8 DC / 1488 GPUs / 8 ingresses",
                "rl_train_steps_per_sec": rl_steps_s,
                "rl_baseline_steps_per_sec": 36.9,
                "rl_loop_events_per_sec": rl_loop_ev_s,
                "rl_loop_updates_per_sec": rl_loop_up_s,
                "rl_loop_baseline_events_per_sec": 127.0,
            },
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()
