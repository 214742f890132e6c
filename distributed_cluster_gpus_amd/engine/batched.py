"""BatchedEngine: MI355X Monte-Carlo replica engine orchestrator.

Allocates the replica-major SoA device state (models/scenario tables +
per-replica simulation state; engine/state.py) as torch tensors on the GPU,
seeds the arrivals, sets up the RL agent and replay, then drives the
gfx950 advance kernel (ops/csrc/hip/replica_engine.hip) in chunks until every
replica reaches end_time.  One wavefront advances one replica; R replicas run
concurrently.  Memory is sized for 288 GB HBM3E — the default 4096-replica
paper-config state is ~2 GB, so tens of thousands of replicas per GPU fit
comfortably (BASELINE.json config 3: 65k replicas over 8 GPUs).

Multi-GPU: replicas are sharded across ranks (parallel/sharding.py); RNG
streams key on GLOBAL replica ids so results are independent of world size;
metric reduction is one small RCCL all-reduce at the end.

Logging: a designated replica (global replica 0, on whichever rank owns it)
records cluster/job rows in device buffers; the host formats them through the
same CSV writers as the scalar engines, so the batched path emits the exact
log schema.  Other replicas contribute to Monte-Carlo aggregate metrics only
— a capability the scalar reference cannot express (SURVEY §6 north-star).

GPU-required: this engine fails loudly if CUDA/ROCm or the _sim_hip extension
is unavailable (no silent CPU fallback).
"""
import math
import os
from typing import Optional

import numpy as np
import torch

from ..models.arrivals import ArrivalProcess
from ..models.scenario import Scenario
from ..ops import load_sim_hip
from ..utils.csvlog import ClusterLogWriter, JobLogWriter
from ..utils.timers import ThroughputMeter
from .oracle import ALGOS
from .state import (ARR_CAP, INF, RL_HID, SERIES_METRICS, alloc_state,
                    engine_cfg, engine_dims, load_tensors)

# the fleet row of the population series (per-DC rows: SERIES_METRICS)
SERIES_FLEET = "ALL"


class BatchedEngine:
    def __init__(self, scenario: Scenario,
                 arrival_inf: ArrivalProcess, arrival_trn: ArrivalProcess,
                 *, algo: str = "default_policy", replicas: int = 4096,
                 duration: float = 3600.0, log_interval: float = 10.0,
                 out_dir: Optional[str] = None, seed: int = 42,
                 power_cap: float = 0.0, control_interval: float = 5.0,
                 elastic_scaling: bool = False, eco_objective: str = "energy",
                 num_fixed_gpus: int = 1, fixed_freq: Optional[float] = None,
                 logger=None, show_progress: bool = False,
                 device: Optional[torch.device] = None,
                 rank: int = 0, world: int = 1,
                 tcap: int = 64, qcap: int = 24576,
                 events_per_launch: int = 50000,
                 enable_logs: bool = True,
                 sla_p99_ms: float = 500.0, energy_budget_j=None,
                 rl_device: str = 'cuda', rl_batch: int = 256,
                 rl_warmup: int = 1000, rl_buffer: int = 200000,
                 rl_train_interval: int = 256, rl_agent=None,
                 rl_stats_interval: int = 100,
                 rl_serve: str = "device", rl_deterministic: bool = False,
                 rl_exact_p99: bool = False, fp32_coeff_eval: bool = False,
                 rl_tr_limit: Optional[int] = None, rl_reserve_cus: int = 16,
                 rl_target_updates_per_s: float = 180.0,
                 tr_cap: int = 262144, arrival_trace=None,
                 subwave: int = 64,
                 pop_series: bool = False, pop_series_every: int = 1,
                 arrival_pregen: bool = True, arr_cap: int = ARR_CAP,
                 **_unused):
        if algo not in ALGOS:
            raise ValueError(f"unknown algo {algo!r}")
        if pop_series and int(pop_series_every) < 1:
            raise ValueError("pop_series_every must be >= 1")
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedEngine requires a ROCm GPU "
                               "(no silent CPU fallback)")
        # subwave=64: one wavefront per replica (default);
        # subwave=8: eight replicas per wavefront (mw variant)
        self._mod = load_sim_hip("_sim_hip" if subwave == 64 else "_sim_hip_mw")
        self.sc = scenario
        self.algo = algo
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.end_time = float(duration)
        self.log_interval = float(log_interval)
        self.events_per_launch = int(events_per_launch)
        self.out_dir = out_dir
        self.rl = None
        self.replay = None
        self.rank = int(rank)
        self.world = int(world)
        self.logger = logger

        from ..parallel.sharding import replica_shard
        shard = replica_shard(int(replicas), rank, world)
        self.shard = shard
        R = shard.count
        self.R = R
        n_dc = scenario.n_dc
        n_g = int(scenario.policy.max_gpus_per_job)
        dev = self.device

        # logging: global replica 0 lives on the rank-0 shard
        self.log_replica = 0 if (enable_logs and shard.start == 0) else -1
        self._jl_chunks = []  # host-side drained job-row chunks (np arrays)
        self.pop_series = bool(pop_series)
        self.pop_series_every = int(pop_series_every) if self.pop_series else 0
        self.trace_mode = arrival_trace is not None

        # ===== CHSAC-AF (RL-in-the-loop) =====
        self.is_rl = algo == "chsac_af"
        obs_dim = 1 + 6 * n_dc
        self.obs_dim = obs_dim
        self.sla_p99_ms = float(sla_p99_ms)
        self._rl_batch = int(rl_batch)
        self._rl_warmup = int(rl_warmup)
        self._rl_train_interval = int(rl_train_interval)
        self._rl_stats_interval = int(rl_stats_interval)
        self._rl_det = bool(rl_deterministic)
        self._rl_hid = RL_HID
        self.rl_updates = 0
        # serving mode: "device" = the actor MLP + masked Gumbel-max sampling
        # run INSIDE the advance kernel from a flat weights buffer (replicas
        # never pause for a host policy round-trip — the round-1 206k ev/s
        # bottleneck); "host" = pause/resume with a batched torch forward
        # (used for parity testing and injected non-standard agents)
        self._serve_device = self.is_rl and rl_serve == "device"
        # the flat buffer also feeds the MFMA batched forward used by the
        # host-serving path (matrix-core policy evaluation)
        self._mfma_serve = False
        self._reserve_cus = int(rl_reserve_cus)
        # overlapped-loop update-rate target: after each advance window the
        # cycle trains serially until the measured SAC update rate meets
        # this (<=0 disables the controller: throughput mode, training is
        # purely opportunistic).  The standalone hipGraph rate is ~227/s;
        # 180 keeps >1M events/s alongside (measured curve in
        # profiles/README.md: 199 -> 0.74M, 188 -> 0.91M, 149 -> 2.1M,
        # throughput mode -> 5.4M ev/s).
        self._rl_target_ups = float(rl_target_updates_per_s)
        if self.is_rl:
            # agent + replay on the same device
            from ..rl.agent import CHSACAgentConfig, make_agent
            from ..rl.replay import ReplayRing
            constraints = {"latency_p99": self.sla_p99_ms}
            if power_cap and power_cap > 0:
                constraints["power"] = float(power_cap)
            if energy_budget_j and energy_budget_j > 0:
                constraints["energy_total"] = float(energy_budget_j)
            constraints["gpu_over"] = 0.0
            self._cost_names = ["latency_p99", "power", "gpu_over"]
            if rl_agent is not None:
                self.rl = rl_agent
            else:
                self.rl = make_agent(CHSACAgentConfig(
                    obs_dim=obs_dim, n_dc=n_dc, n_g_choices=n_g,
                    constraints=constraints, device=str(dev),
                    graph_capturable=(world == 1)))
            self._graphed = None
            self._use_graph = (world == 1 and rl_agent is None)
            self.replay = ReplayRing(capacity=int(rl_buffer), obs_dim=obs_dim,
                                     n_costs=3, cost_names=self._cost_names,
                                     n_dc=n_dc, n_g=n_g,
                                     device=str(dev), seed=seed)
            servable = self._actor_is_servable(self._rl_hid)
            if self._serve_device and not servable:
                import warnings
                warnings.warn("injected agent has non-standard actor dims; "
                              "falling back to host policy serving")
                self._serve_device = False
            self._mfma_serve = servable and not self._serve_device \
                and not self._rl_det

        # device state (engine/state.py): sizes once, then the tensors
        dims = engine_dims(
            scenario, algo=algo, n_rep=R, duration=duration,
            log_interval=log_interval, tcap=tcap, qcap=qcap,
            events_per_launch=events_per_launch,
            log_replica=self.log_replica,
            pop_series_every=self.pop_series_every,
            arrival_trace=arrival_trace, power_cap=power_cap,
            eco_objective=eco_objective, fp32_coeff_eval=fp32_coeff_eval,
            num_fixed_gpus=num_fixed_gpus, fixed_freq=fixed_freq, seed=seed,
            rep_id_offset=shard.start, sla_p99_ms=sla_p99_ms, tr_cap=tr_cap,
            elastic_scaling=elastic_scaling, rl_exact_p99=rl_exact_p99,
            serve_device=self._serve_device, weights_buffer=self._mfma_serve,
            rl_deterministic=rl_deterministic, rl_tr_limit=rl_tr_limit,
            rl_train_interval=rl_train_interval,
            # arrivals pre-generated lane-parallel into a per-replica ring
            # (ops/csrc/hip/arrival_ring.hpp); the 8-lane build draws inline
            # and stays the independent reference
            arrival_pregen=bool(arrival_pregen) and subwave == 64,
            arr_cap=arr_cap)
        self.dims = dims
        if self.pop_series:
            ps_bytes = dims.ps_cap * (n_dc + 1) * len(SERIES_METRICS) * R * 8
            import logging
            from ..utils.logging import LOGGER_NAME
            (logger or logging.getLogger(LOGGER_NAME)).info(
                f"pop_series: sample buffer {dims.ps_cap} ticks x {n_dc + 1} "
                f"rows x {len(SERIES_METRICS)} metrics x {R} replicas x 8 B = "
                f"{ps_bytes} bytes ({ps_bytes / 2**20:.1f} MiB)")
        t = alloc_state(dims, scenario, dev, arrival_trace)
        if not self.trace_mode:
            # seed the initial arrival times on host (one inf + one trn per
            # ingress per replica), Philox-consistent with the device streams:
            # the kernel's first draws start at ctr = n_streams; host uses
            # ctr = stream index for the seed draws.
            arr_np = self._seed_arrivals(arrival_inf, arrival_trn, seed, shard)
            t["arr_next"].copy_(torch.as_tensor(arr_np, dtype=torch.float64))
        self.t = t
        self.arrival_inf, self.arrival_trn = arrival_inf, arrival_trn

        self._sim = self._mod.BatchedSimHip(
            t, engine_cfg(dims, scenario, arrival_inf, arrival_trn))
        self.meter = ThroughputMeter()
        if self._serve_device or self._mfma_serve:
            self._build_weight_refs()
            self._refresh_policy_weights()

    def _seed_arrivals(self, arrival_inf, arrival_trn, seed, shard):
        """Host-side Philox draws for the initial inter-arrival per stream,
        matching the device recipe (philox.hpp)."""
        from ._philox_host import philox_u01, replica_key, rexp
        R = shard.count
        NS = self.sc.n_ing * 2
        out = np.full((R, NS), INF)
        for r in range(R):
            key = replica_key(seed, shard.start + r)
            ctr = 0
            for s in range(NS):
                jt = s & 1
                arr = arrival_inf if jt == 0 else arrival_trn
                # the kernel reserves one counter per stream for the seed draw;
                # thinning may need more draws -> sub-counter space: we use
                # counter = stream index, and for extra thinning draws we
                # borrow high bits (replica-unique; never reused by the device
                # which starts at ctr = NS).
                if arr.mode == "off" or arr.rate <= 0:
                    ctr += 1
                    continue
                if arr.mode == "poisson":
                    out[r, s] = rexp(key, ctr, arr.rate)
                    ctr += 1
                else:  # sinusoid thinning at t=0
                    max_rate = arr.rate * (1.0 + abs(arr.amp))
                    sub = 0
                    ia = INF
                    while sub < 4096:
                        w = rexp(key, ctr + ((sub * 2 + 1) << 32), max_rate)
                        lam = max(0.0, arr.rate * (1.0 + arr.amp * math.sin(
                            2.0 * math.pi * (w % arr.period) / arr.period)))
                        u2 = philox_u01(key, ctr + ((sub * 2 + 2) << 32))
                        if u2 <= lam / max_rate:
                            ia = w
                            break
                        sub += 1
                    out[r, s] = ia
                    ctr += 1
        return out

    # ---------------- run ----------------
    def run(self, max_wall_s: Optional[float] = None):
        """Drive advance launches until every replica reaches end_time (or
        `max_wall_s` of wall clock passes — benchmarking aid).

        Single-GPU chsac with in-kernel serving runs the OVERLAPPED loop:
        the advance kernel executes on its own HIP stream while SAC train
        steps replay on the default stream, so training no longer serializes
        with simulation; the serving weight buffer refreshes only between
        launches (the kernel never reads a half-copied buffer).  Training is
        then paced opportunistically (as many updates as fit under the
        advance window) — with thousands of replicas the effective
        samples-trained-per-transition ratio stays ~1 like the
        interval-paced cadence, but wall-clock decouples.

        Data-parallel mode (world > 1 with torch.distributed initialized):
        every rank executes the SAME number of loop iterations and, inside
        each, the SAME number of SAC train steps — the per-launch step count
        is derived from globally reduced counters (parallel/dist.py
        ``dp_sync_step``), so the gradient/cost all-reduces inside
        ``train_step`` are structurally paired and no rank can hang waiting
        for a peer that finished early (round-1 advisor finding)."""
        self.meter.start()
        t = self.t
        from ..parallel.dist import dp_sync_step, is_distributed
        dp = self.is_rl and self.world > 1 and is_distributed()
        overlap = self.is_rl and not dp and self._serve_device
        if overlap:
            # The advance kernel's blocks are persistent for a whole cycle, so
            # an unmasked launch occupies every wave slot and concurrent train
            # kernels starve (measured: 38 updates/s).  Reserve a small CU
            # island via a CU-masked stream: the advance never dispatches
            # there, and the train stream's kernels land immediately.
            try:
                self._sim.enable_masked_stream(self._reserve_cus)
            except RuntimeError as e:
                # masked stream unavailable: overlap still works, slower
                import warnings
                warnings.warn(f"CU-masked stream unavailable ({e}); "
                              "train kernels may contend with the advance "
                              "kernel")
            # train on a torch-created (NON-BLOCKING) stream: the masked
            # stream is a blocking stream, and the legacy NULL stream
            # implicitly synchronizes with all blocking streams — training
            # on the default stream would serialize behind every advance
            # launch (measured: exactly floor+1 steps/cycle at every island
            # size).  Two non-NULL streams have no implicit ordering.
            self._train_stream = torch.cuda.Stream(device=self.device)
        launches = 0
        self._tr_backlog = 0  # transitions not yet converted into train steps
        self._ups_t0 = None   # update-rate controller epoch (first trainable)
        import time as _time
        tm = {"advance_s": 0.0, "serve_s": 0.0, "dp_sync_s": 0.0,
              "train_s": 0.0, "overlap_train_steps": 0, "launches": 0,
              "sync0_s": 0.0, "kernel_s": 0.0, "status_s": 0.0,
              "ingest_s": 0.0, "floor_s": 0.0, "refresh_s": 0.0}
        self.timing = tm
        wall0 = _time.perf_counter()
        while True:
            if overlap:
                if self._run_cycle_overlapped(tm, _time):
                    break
                launches += 1
                tm["launches"] = launches
                if launches > 1000000:
                    raise RuntimeError("batched engine failed to converge")
                if max_wall_s and _time.perf_counter() - wall0 > max_wall_s:
                    break
                continue
            t0 = _time.perf_counter()
            self._sim.advance(self.end_time, self.events_per_launch)
            launches += 1
            tm["launches"] = launches
            # one fused D2H status read per launch (err / done / pending /
            # transitions / job-log rows) instead of several .item() syncs
            status = torch.stack([
                t["err"].max(),
                t["done"].min(),
                (t["req_flag"] == 1).sum().to(torch.int32) if self.is_rl
                else torch.zeros((), dtype=torch.int32, device=self.device),
                t["tr_count"][0] if self.is_rl
                else torch.zeros((), dtype=torch.int32, device=self.device),
                t["jl_count"][0],
            ]).cpu()
            err = int(status[0])
            local_done = int(status[1]) == 1
            t1 = _time.perf_counter()
            tm["advance_s"] += t1 - t0
            if err != 0 and not dp:
                # before serving or ingesting anything the overflowed launch
                # produced (dp: every rank raises together after the sync)
                raise RuntimeError(
                    f"batched engine error flags: {err:#x} "
                    f"(queue/transfer/slot/log overflow)")
            if int(status[4]) >= int(t["jl_rows"].shape[0]) // 2:
                self._drain_job_rows()
            n_new = 0
            if self.is_rl:
                self._rl_serve(n_req=int(status[2]))
                n_new = self._rl_ingest(n_tr=int(status[3]))
            t2 = _time.perf_counter()
            tm["serve_s"] += t2 - t1
            if dp:
                err_g, all_done, min_replay, tr_total = dp_sync_step(
                    err, local_done, self.replay.size, n_new)
                tm["dp_sync_s"] += _time.perf_counter() - t2
                if err_g != 0:
                    raise RuntimeError(
                        f"batched engine error flags (some rank): {err_g:#x}")
                self._tr_backlog += tr_total
                steps = 0
                if min_replay >= max(self._rl_warmup, self._rl_batch):
                    per_step = self._rl_train_interval * self.world
                    steps = min(64, self._tr_backlog // per_step)
                    self._tr_backlog -= steps * per_step
                t3 = _time.perf_counter()
                self._rl_train(steps)
                tm["train_s"] += _time.perf_counter() - t3
                if all_done:
                    break
            else:
                if self.is_rl:
                    self._tr_backlog += n_new
                    steps = 0
                    if self.replay.size >= self._rl_warmup:
                        steps = min(64, self._tr_backlog // self._rl_train_interval)
                        self._tr_backlog -= steps * self._rl_train_interval
                    t3 = _time.perf_counter()
                    self._rl_train(steps)
                    tm["train_s"] += _time.perf_counter() - t3
                if local_done:
                    break
            if launches > 1000000:
                raise RuntimeError("batched engine failed to converge")
            if max_wall_s and _time.perf_counter() - wall0 > max_wall_s:
                break
        self.meter.count = int(t["ev_count"].sum().item())
        self.meter.stop()
        if self.log_replica >= 0 and self.out_dir is not None:
            self._write_logs()
        return self.stats()

    def _run_cycle_overlapped(self, tm, _time):
        """One overlapped cycle: advance on the CU-masked stream, SAC updates
        on the torch default stream (which owns the reserved CU island) while
        the kernel runs, then sync / ingest / refresh.  A small serial floor
        (up to 4 interval-paced steps per cycle) guarantees short runs still
        train even when the whole simulation fits in one cycle.
        Returns True when every replica is done."""
        t = self.t
        t0 = _time.perf_counter()
        # the kernel must see last cycle's weight refresh / tr_count reset
        torch.cuda.current_stream(self.device).synchronize()
        tm["sync0_s"] += _time.perf_counter() - t0
        tk = _time.perf_counter()
        self._sim.advance(self.end_time, self.events_per_launch)
        # train under the advance window (one graph replay at a time, synced
        # so host pacing tracks device completion)
        t1 = _time.perf_counter()
        can_train = (self.replay.size >=
                     max(self._rl_warmup, self._rl_batch))
        trained = 0
        if can_train:
            ts = self._train_stream
            ts.wait_stream(torch.cuda.current_stream(self.device))
            while trained < 1024 and not self._sim.advance_done():
                with torch.cuda.stream(ts):
                    self._rl_train(1, refresh=False)
                ts.synchronize()
                trained += 1
        self._sim.advance_sync()
        tm["kernel_s"] += _time.perf_counter() - tk
        if can_train:
            # later default-stream ops (floor steps, refresh) must see the
            # side-stream parameter updates
            torch.cuda.current_stream(self.device).wait_stream(
                self._train_stream)
        tm["train_s"] += _time.perf_counter() - t1
        t2 = _time.perf_counter()
        status = torch.stack([
            t["err"].max(),
            t["done"].min(),
            t["tr_count"][0],
            t["jl_count"][0],
        ]).cpu()
        err = int(status[0])
        if err != 0:
            raise RuntimeError(f"batched engine error flags: {err:#x} "
                               f"(queue/transfer/slot/log overflow)")
        tm["status_s"] += _time.perf_counter() - t2
        if int(status[3]) >= int(t["jl_rows"].shape[0]) // 2:
            self._drain_job_rows()
        t3 = _time.perf_counter()
        self._rl_ingest(n_tr=int(status[2]))
        tm["ingest_s"] += _time.perf_counter() - t3
        # update-rate controller: train serially until the measured update
        # rate meets the target (the advance kernel's oversubscribed grid
        # head-of-line-blocks concurrent dispatch, so opportunistic overlap
        # alone cannot sustain the standalone train rate — measured)
        t4 = _time.perf_counter()
        if self.replay.size >= max(self._rl_warmup, self._rl_batch):
            if self._ups_t0 is None:
                self._ups_t0 = _time.perf_counter()
                self._ups_base = self.rl_updates
            tgt = self._rl_target_ups
            extra = 0
            while tgt > 0 and extra < 64:
                el = max(1e-6, _time.perf_counter() - self._ups_t0)
                if (self.rl_updates - self._ups_base) >= tgt * el:
                    break
                self._rl_train(1, refresh=False)
                extra += 1
            trained += extra
        tm["floor_s"] += _time.perf_counter() - t4
        tm["overlap_train_steps"] += trained
        t5 = _time.perf_counter()
        self._refresh_policy_weights()
        tm["refresh_s"] += _time.perf_counter() - t5
        tm["advance_s"] += _time.perf_counter() - t0
        return int(status[1]) == 1

    def _drain_job_rows(self):
        """Chunk-wise drain of the device job-log buffer so unboundedly many
        job rows stream to the host (the reference streams rows to CSV
        unboundedly, simulator_paper_multi.py:814-823)."""
        t = self.t
        n = int(t["jl_count"].item())
        if n > 0:
            self._jl_chunks.append(t["jl_rows"][:n].cpu().numpy().copy())
            t["jl_count"].zero_()

    # ---------------- CHSAC host service ----------------
    def _expand_mask(self, bytes_tensor, width):
        """uint8/int bitmask tensor [B] -> bool [B, width]."""
        b = bytes_tensor.to(torch.int64).unsqueeze(1)
        return (b >> torch.arange(width, device=b.device).unsqueeze(0)) & 1 > 0

    def _rl_serve(self, n_req=None):
        """Serve pending action requests with ONE batched policy forward."""
        t = self.t
        pend = t["req_flag"] == 1
        if n_req is None:
            n_req = int(pend.sum().item())
        if n_req <= 0:
            return
        idx = pend.nonzero(as_tuple=True)[0]
        obs = t["req_obs"][idx]
        n_dc = self.sc.n_dc
        n_g = int(self.sc.policy.max_gpus_per_job)
        m_dc = self._expand_mask(t["req_mdc"][idx], n_dc)
        m_g = self._expand_mask(t["req_mg"][idx], n_g)
        # guard: a fully-false mask wedges the categorical; allow all
        m_dc[m_dc.sum(dim=1) == 0] = True
        m_g[m_g.sum(dim=1) == 0] = True
        if self._rl_det:
            # parity mode: serve one request at a time through the SAME
            # scalar entry the oracle uses, so batch-size-dependent GEMM
            # reduction order can never flip a near-tie argmax
            obs_np = obs.cpu().numpy()
            mdc_np = m_dc.cpu().numpy()
            mg_np = m_g.cpu().numpy()
            dcs, gs = [], []
            for i in range(obs_np.shape[0]):
                a = self.rl.select_action(obs_np[i], mdc_np[i], mg_np[i],
                                          deterministic=True)
                dcs.append(a["dc"])
                gs.append(a["g"])
            t["resp_dc"][idx] = torch.as_tensor(dcs, dtype=torch.int32,
                                                device=self.device)
            t["resp_g"][idx] = torch.as_tensor(gs, dtype=torch.int32,
                                               device=self.device)
        elif self._mfma_serve:
            # matrix-core batched forward (rl_forward_mfma) + the same
            # masked Gumbel-max sampling the torch path uses
            from ..rl.masking import sample_categorical
            with torch.no_grad():
                ldc, lg = self._mod.rl_forward_mfma(
                    t["policy_weights"], obs.contiguous(),
                    self._rl_hid, n_dc, n_g)
                a_dc, _ = sample_categorical(ldc, m_dc)
                a_g, _ = sample_categorical(lg, m_g)
            t["resp_dc"][idx] = a_dc.to(torch.int32)
            t["resp_g"][idx] = a_g.to(torch.int32)
        else:
            with torch.no_grad():
                a = self.rl.select_action_batch(obs, m_dc, m_g)
            t["resp_dc"][idx] = a["dc"].to(torch.int32)
            t["resp_g"][idx] = a["g"].to(torch.int32)
        t["req_flag"][idx] = 2  # REQ_READY

    def _rl_ingest(self, n_tr=None) -> int:
        """Drain completed transitions from the device ring into the replay
        ring; returns the number ingested."""
        t = self.t
        if n_tr is None:
            n_tr = int(t["tr_count"].item())
        if n_tr <= 0:
            return 0
        n_tr = min(n_tr, int(t["tr_s0"].shape[0]))
        costs = t["tr_costs"][:n_tr]
        self.replay.add_batch(
            s=t["tr_s0"][:n_tr], s_next=t["tr_s1"][:n_tr],
            a_dc=t["tr_adc"][:n_tr].to(torch.long),
            a_g=t["tr_ag"][:n_tr].to(torch.long),
            r=t["tr_r"][:n_tr], costs=costs,
            done=torch.ones(n_tr, device=self.device),
            mask_dc=self._expand_mask(t["tr_mdc"][:n_tr], self.sc.n_dc),
            mask_g=self._expand_mask(t["tr_mg"][:n_tr],
                                     int(self.sc.policy.max_gpus_per_job)))
        t["tr_count"].zero_()
        return n_tr

    def _rl_train(self, steps: int, refresh: bool = True):
        """Run `steps` SAC updates: hipGraph-replayed when captured, eager
        otherwise.  Every `rl_stats_interval`-th update runs eagerly with
        compute_stats=True and logs losses/alpha/lambda at INFO — the
        batched-path equivalent of the reference's per-update INFO logging
        (simulator_paper_multi.py:755,807; sampled here because production
        updates are graph-replayed and sync-free).  refresh=False defers the
        serving-buffer update to the caller (the overlapped loop refreshes
        only after the concurrent advance kernel has finished, so the kernel
        never reads a half-copied weight buffer)."""
        if steps <= 0:
            return
        if self._use_graph and self._graphed is None:
            from ..rl.graphed import GraphedSACStep
            self._graphed = GraphedSACStep(self.rl, self.replay, self._rl_batch)
        for _ in range(steps):
            self.rl_updates += 1
            want_stats = (self._rl_stats_interval > 0 and self.logger is not None
                          and (self.rl_updates == 1 or
                               self.rl_updates % self._rl_stats_interval == 0))
            if want_stats:
                stats = self.rl.train_step(self.replay.sample(self._rl_batch),
                                           compute_stats=True)
                self.logger.info(
                    {"rl_update": self.rl_updates,
                     **{k: round(v, 4) if isinstance(v, (int, float)) else v
                        for k, v in stats.items()}})
            elif self._graphed is not None:
                self._graphed.step()  # one hipGraph replay
            else:
                # sync-free eager SAC step (no stats, tensorized PID)
                self.rl.train_step(self.replay.sample(self._rl_batch),
                                   compute_stats=False)
        if refresh and (self._serve_device or
                        self._mfma_serve):
            self._refresh_policy_weights()

    # ---- in-kernel serving support ----
    def _actor_lins(self):
        """The 7 Linear layers of the served actor, in buffer-layout order."""
        rl = self.rl
        enc = rl.encoder.net
        return [enc[0], enc[2], enc[4],
                rl.actor.head_dc[0], rl.actor.head_dc[2],
                rl.actor.head_g[0], rl.actor.head_g[2]]

    def _actor_is_servable(self, H: int) -> bool:
        try:
            lins = self._actor_lins()
        except (AttributeError, IndexError, TypeError):
            return False
        shapes = [tuple(l.weight.shape) for l in lins]
        n_dc = self.sc.n_dc
        n_g = int(self.sc.policy.max_gpus_per_job)
        want = [(H, self.obs_dim), (H, H), (H, H),
                (H, H), (n_dc, H), (H, H), (n_g, H)]
        return shapes == want and n_dc <= 8 and n_g <= 8 and self.obs_dim <= 64

    def _build_weight_refs(self):
        """Precompute (buffer-slice view, source-parameter) pairs so each
        refresh is a handful of small device-to-device copies."""
        buf = self.t["policy_weights"]
        pairs = []
        off = 0
        for lin in self._actor_lins():
            w = lin.weight          # [out, in] -> stored transposed [in][out]
            n = w.numel()
            pairs.append((buf[off:off + n].view(w.shape[1], w.shape[0]), w))
            off += n
            b = lin.bias
            pairs.append((buf[off:off + b.numel()], b))
            off += b.numel()
        assert off == buf.numel(), (off, buf.numel())
        self._w_pairs = pairs

    @torch.no_grad()
    def _refresh_policy_weights(self):
        """Push the current actor weights into the kernel's serving buffer
        (called after every train round; bounds policy staleness together
        with the kernel's tr_limit launch yield)."""
        for dst, src in self._w_pairs:
            dst.copy_(src.t() if dst.dim() == 2 else src)

    def _rl_service(self, n_req=None, n_tr=None):
        """Back-compat single-rank service entry (serve + ingest + local-
        cadence training); the run() loop calls the split methods directly."""
        self._rl_serve(n_req)
        n_new = self._rl_ingest(n_tr)
        self._tr_backlog = getattr(self, "_tr_backlog", 0) + n_new
        steps = 0
        if self.replay is not None and self.replay.size >= self._rl_warmup:
            steps = min(64, self._tr_backlog // self._rl_train_interval)
            self._tr_backlog -= steps * self._rl_train_interval
        self._rl_train(steps)

    def stats(self):
        t = self.t
        jobs = int(t["jobs_done"].sum().item())
        jobs_inf = int(t["jobs_done_inf"].sum().item())
        stats = {
            "events": int(t["ev_count"].sum().item()),
            "wall_s": self.meter.elapsed_s,
            "events_per_sec": self.meter.per_sec,
            "rl_updates": self.rl_updates,
            "jobs_completed": jobs,
            "jobs_completed_inf": jobs_inf,
            "replicas": self.R,
            "total_energy_j": float(t["energy_j"].sum().item()),
            "mean_energy_j_per_replica": float(t["energy_j"].sum().item()) / max(1, self.R),
            "energy_j_replica_std": float(t["energy_j"].sum(dim=1).std().item()) if self.R > 1 else 0.0,
            "mean_latency_s": float(t["sum_lat"].sum().item()) / max(1, jobs),
            "mean_inf_latency_s": (float(t["sum_lat_inf"].sum().item()) / max(1, jobs_inf)),
            "mean_wait_s": float(t["sum_wait"].sum().item()) / max(1, jobs),
            "launches": 0,
        }
        return stats

    def metrics_tensors(self):
        """Raw per-replica metric tensors (for cross-rank RCCL reductions)."""
        t = self.t
        return {k: t[k] for k in ("ev_count", "jobs_done", "jobs_done_inf",
                                  "sum_lat", "sum_lat_inf", "energy_j")}

    # ---------------- population time series ----------------
    def pop_samples(self):
        """Raw device views of the population time series: ``samples``
        [T_cap, n_dc+1, K, R] (row n_dc = fleet), ``ticks`` [R] (log ticks
        each replica has processed) and ``time`` [T_cap] (tick times)."""
        if not self.pop_series:
            raise RuntimeError("engine was built without pop_series=True")
        t = self.t
        return {"samples": t["ps_samples"], "ticks": t["ps_tick"],
                "time": t["ps_time"]}

    def population_series(self):
        """Per-tick statistics over the replica ensemble as a SeriesStats
        (analysis/montecarlo.py): n, mean, M2, min, max of every sampled
        metric per DC and fleet-wide, trimmed to the ticks at least one
        replica has reached.  Valid on an unfinished run (n counts the
        replicas that reached each tick).  Under torch.distributed the
        per-rank statistics are merged, so every rank holds the global
        series."""
        from ..analysis.montecarlo import SeriesStats, merge_series_stats
        from ..parallel.dist import allgather_series_stats, is_distributed
        ps = self.pop_samples()
        every = self.pop_series_every
        cap = int(ps["samples"].shape[0])
        dist_on = self.world > 1 and is_distributed()
        # ranks must agree on the shape they gather: the full buffer then
        T = cap if dist_on else min(cap, int(ps["ticks"].max().item()) // every)
        n_row, K = self.sc.n_dc + 1, len(SERIES_METRICS)
        raw = self._mod.reduce_series(
            ps["samples"][:T].view(T, n_row * K, self.R), ps["ticks"], every)
        names = list(self.sc.dc_names) + [SERIES_FLEET]

        def wrap(flat_stats, time):
            return SeriesStats.from_tensor(
                flat_stats.view(T, n_row, K, 5), time,
                metrics=list(SERIES_METRICS), dc_names=names)

        if not dist_on:
            return wrap(raw.cpu(), ps["time"][:T].cpu()).trimmed()
        flat = torch.cat([raw.reshape(-1), ps["time"][:T]])
        parts = [p.cpu() for p in allgather_series_stats(flat)]
        return merge_series_stats(
            [wrap(p[:-T], p[-T:]) for p in parts]).trimmed()

    # ---------------- state checkpointing (capability extension) ----------
    def save_state(self, path: str):
        """Checkpoint the COMPLETE engine state (every device tensor plus the
        host cursor scalars) so a long Monte-Carlo run can resume exactly.
        The reference has no simulator-state checkpointing at all
        (SURVEY §5 'Checkpoint/resume')."""
        torch.save({"tensors": {k: v.cpu() for k, v in self.t.items()},
                    "meter_count": self.meter.count,
                    "rl_updates": self.rl_updates,
                    "jl_chunks": self._jl_chunks,
                    "rl": self.rl.state_dict() if self.rl is not None else None},
                   path)

    def load_state(self, path: str):
        st = torch.load(path, map_location="cpu", weights_only=False)
        load_tensors(self.t, st["tensors"])
        self.rl_updates = st.get("rl_updates", 0)
        self._jl_chunks = list(st.get("jl_chunks", []))
        if self.rl is not None and st.get("rl") is not None:
            self.rl.load_state_dict(st["rl"])

    # ---------------- invariant validation (race detection) ---------------
    def validate_state(self):
        """Cross-check the engine's cached/derived state against first
        principles with torch reductions — the batched engine's race/corruption
        detector (SURVEY §5 'Race detection': the slot allocator and caches are
        the racy-by-construction parts; this validates them after any run).
        Raises AssertionError on violation."""
        t = self.t
        n_dc = self.sc.n_dc
        slot_dc = t["slot_dc"].long()
        gpus = t["s_gpus"].long()                       # [R, slots]
        active = gpus > 0
        # busy[r,d] == sum of gpus over active slots of DC d
        busy_ref = torch.zeros((self.R, n_dc), dtype=torch.long,
                               device=self.device)
        busy_ref.scatter_add_(1, slot_dc.unsqueeze(0).expand(self.R, -1), gpus)
        assert torch.equal(busy_ref, t["busy"].long()), "busy != sum(slot gpus)"
        # n_running[r,d] == count of active slots
        run_ref = torch.zeros((self.R, n_dc), dtype=torch.long,
                              device=self.device)
        run_ref.scatter_add_(1, slot_dc.unsqueeze(0).expand(self.R, -1),
                             active.long())
        assert torch.equal(run_ref, t["n_running"].long()),             "n_running != active slot count"
        # busy never exceeds capacity; queue lengths within bounds
        assert bool((t["busy"] <= t["total_gpus"].unsqueeze(0)).all()),             "busy > total_gpus"
        # (queue_push refuses at q_len >= qcap, so a full ring holds qcap)
        assert bool((t["q_len"] >= 0).all()) and \
            bool((t["q_len"] <= t["q_pay"].shape[-2]).all()), \
            "q_len outside [0, qcap]"
        # empty slots hold +inf finish; active slots hold finite times
        fin = t["s_finish"]
        assert bool((fin[~active] >= INF).all()), "empty slot with finite finish"
        assert bool((fin[active] < INF).all()), "active slot with inf finish"
        # energy monotone non-negative
        assert bool((t["energy_j"] >= 0).all())
        assert int(t["err"].max().item()) == 0
        return True

    # ---------------- log formatting ----------------
    def _write_logs(self):
        t = self.t
        os.makedirs(self.out_dir, exist_ok=True)
        cw = ClusterLogWriter(os.path.join(self.out_dir, "cluster_log.csv"))
        n_cl = int(t["cl_count"].item())
        rows = t["cl_rows"][:n_cl].cpu().numpy()
        for row in rows:
            d = int(row[1])
            cw.row(row[0], self.sc.dc_names[d], row[2], int(row[3]), int(row[4]),
                   int(row[5]), int(row[6]), int(row[7]), int(row[8]), int(row[9]),
                   row[10], row[11], row[12], row[13], row[14])
        cw.close()
        jw = JobLogWriter(os.path.join(self.out_dir, "job_log.csv"))
        n_jl = int(t["jl_count"].item())
        chunks = list(self._jl_chunks)
        if n_jl > 0:
            chunks.append(t["jl_rows"][:n_jl].cpu().numpy())
        jrows = np.concatenate(chunks, axis=0) if chunks else \
            np.zeros((0, t["jl_rows"].shape[1]))
        from ..models.coeffs import LatencyCoeffs, PowerCoeffs
        from ..policies.gridsearch import energy_tuple
        for row in jrows:
            (jid, ing, jt, size, d, fused, n, netlat, start, finish,
             pcount) = row
            d = int(d)
            jt = int(jt)
            pC = PowerCoeffs(*self.sc.power_coeffs[d, jt, :])
            tC = LatencyCoeffs(*self.sc.latency_coeffs[d, jt, :])
            T_pred, P_pred, E_pred = energy_tuple(int(n), float(fused), pC, tC)
            jw.row(int(jid), self.sc.ingress_names[int(ing)],
                   "inference" if jt == 0 else "training", float(size),
                   self.sc.dc_names[d], float(fused), int(n), float(netlat),
                   float(start), float(finish), int(pcount),
                   T_pred, P_pred, E_pred)
        jw.close()
