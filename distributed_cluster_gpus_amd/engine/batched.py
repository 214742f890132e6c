"""BatchedEngine: MI355X Monte-Carlo replica engine orchestrator.

Allocates the replica-major SoA device state (models/scenario tables +
per-replica simulation state; engine/state.py) as torch tensors on the GPU,
seeds the arrivals, then drives the gfx950 advance kernel
(ops/csrc/hip/replica_engine.hip) in chunks until every replica reaches
end_time; for chsac_af the host side of each chunk (serving, replay ingest,
SAC training) is engine/rl_loop.py's.  One wavefront advances one replica; R replicas run
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
import logging
import math
import os
import time
from typing import Optional

import numpy as np
import torch

from ..models.arrivals import ArrivalProcess
from ..models.scenario import Scenario
from ..ops import load_sim_hip
from ..utils.csvlog import ClusterLogWriter, JobLogWriter
from ..utils.logging import LOGGER_NAME
from ..utils.timers import Lap, ThroughputMeter
from .oracle import ALGOS
from .state import (ARR_CAP, INF, LH_BINS, RL_HID, SERIES_METRICS,
                    alloc_state, engine_cfg, engine_dims, load_tensors,
                    profile_table, validate_profile_engine)

# the fleet row of the population series (per-DC rows: SERIES_METRICS)
SERIES_FLEET = "ALL"

# what a cycle may ask of the state after a launch, each one device scalar
_STATUS = {
    "err": lambda t: t["err"].max(),        # overflow flags of any replica
    "done": lambda t: t["done"].min(),      # 1 = every replica finished
    "n_tr": lambda t: t["tr_count"][0],     # transitions in the device ring
    "n_jl": lambda t: t["jl_count"][0],     # buffered job-log rows
    # parked action requests (host serving only)
    "n_req": lambda t: (t["req_flag"] == 1).sum().to(torch.int32),
}


def read_status(t, entries):
    """The named ``_STATUS`` entries as host ints, through ONE fused D2H read
    per launch instead of several .item() syncs.  Only what is named is
    computed."""
    vals = torch.stack([_STATUS[e](t) for e in entries]).cpu().tolist()
    return dict(zip(entries, vals))


def raise_on_err(err: int, some_rank: bool = False):
    if err != 0 and some_rank:
        raise RuntimeError(
            f"batched engine error flags (some rank): {err:#x}")
    if err != 0:
        raise RuntimeError(f"batched engine error flags: {err:#x} "
                           f"(queue/transfer/slot/log overflow)")


def raise_on_group_err(err_per_replica, sweep, shard):
    """``raise_on_err`` for a sweep engine: the same failure, naming the
    groups whose replicas carry error flags (the hottest point of a load
    sweep is the one that overflows ``qcap``).  ``err_per_replica`` is this
    rank's ``err`` tensor or array."""
    err = np.asarray(err_per_replica.cpu() if hasattr(err_per_replica, "cpu")
                     else err_per_replica)
    if not err.any():
        return
    bad = []
    for g in range(sweep.n_groups):
        a, b = sweep.slice_of(g, shard)
        flags = int(np.bitwise_or.reduce(err[a:b])) if b > a else 0
        if flags:
            bad.append(f"group {g} ({sweep.point(g)}): {flags:#x} on "
                       f"{int((err[a:b] != 0).sum())} of {b - a} replicas")
    raise RuntimeError(
        f"batched engine error flags: {int(np.bitwise_or.reduce(err)):#x} "
        "(queue/transfer/slot/log overflow) in sweep " + "; ".join(bad))


def seed_arrivals(n_ing, procs_of_replica, seed, shard):
    """Host-side Philox draws for the initial inter-arrival per stream,
    matching the device recipe (philox.hpp).  ``procs_of_replica(r)`` is
    local replica r's ``(arrival_inf, arrival_trn)``: one shared pair for a
    uniform engine, the replica's own parameters under a sweep."""
    from ._philox_host import (draw_profile_gap, philox_u01, replica_key,
                               rexp)
    R = shard.count
    NS = n_ing * 2
    out = np.full((R, NS), INF)
    for r in range(R):
        key = replica_key(seed, shard.start + r)
        arrival_inf, arrival_trn = procs_of_replica(r)
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
            elif arr.mode == "profile":
                # one unit exponential at ctr = stream index, inverted
                # through the stream's own row at t = 0 (D_INF: a row of 0s)
                out[r, s] = draw_profile_gap(
                    key, ctr, 0.0, arr.rate, arr.period,
                    *arr._table(s >> 1))[0]
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
                 latency_hist: bool = False,
                 latency_sla_s: Optional[float] = None,
                 sweep=None,
                 **_unused):
        if algo not in ALGOS:
            raise ValueError(f"unknown algo {algo!r}")
        if pop_series and int(pop_series_every) < 1:
            raise ValueError("pop_series_every must be >= 1")
        # parameter sweep (engine/sweep.py): G groups of replicas, each at
        # its own arrival parameters / power cap
        self.sweep = sweep
        self.sweep_base = None
        if sweep is not None:
            from .sweep import SweepBase
            self.sweep_base = SweepBase.of(arrival_inf, arrival_trn, power_cap)
            sweep.validate(base=self.sweep_base, algo=algo,
                           replicas=int(replicas),
                           arrival_trace=arrival_trace,
                           arrival_pregen=bool(arrival_pregen),
                           subwave=subwave)
        # per-ingress rate profiles (models/arrivals.py): checked here, before
        # anything touches the GPU
        profile_on = validate_profile_engine(
            arrival_inf, arrival_trn, scenario.n_ing, algo=algo,
            subwave=subwave, arrival_pregen=bool(arrival_pregen),
            arrival_trace=arrival_trace)
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

        # ===== CHSAC-AF (RL-in-the-loop): engine/rl_loop.py =====
        self.is_rl = algo == "chsac_af"
        obs_dim = 1 + 6 * n_dc
        self.obs_dim = obs_dim
        self.sla_p99_ms = float(sla_p99_ms)
        self._rl_drv = None
        serve_device = mfma_serve = False
        if self.is_rl:
            from . import rl_loop
            self.rl, self.replay = rl_loop.make_learner(
                obs_dim, n_dc, n_g, dev, world=world, seed=seed,
                buffer=rl_buffer, sla_p99_ms=sla_p99_ms, power_cap=power_cap,
                energy_budget_j=energy_budget_j, agent=rl_agent)
            serve_device, mfma_serve = rl_loop.serving_mode(
                self.rl, obs_dim, n_dc, n_g, RL_HID, rl_serve,
                bool(rl_deterministic))

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
            serve_device=serve_device, weights_buffer=mfma_serve,
            rl_deterministic=rl_deterministic, rl_tr_limit=rl_tr_limit,
            rl_train_interval=rl_train_interval,
            # arrivals pre-generated lane-parallel into a per-replica ring
            # (ops/csrc/hip/arrival_ring.hpp); the 8-lane build draws inline
            # and stays the independent reference
            arrival_pregen=bool(arrival_pregen) and subwave == 64,
            arr_cap=arr_cap, latency_hist=latency_hist,
            latency_sla_s=latency_sla_s, sweep=sweep,
            arrivals=(arrival_inf, arrival_trn))
        self.dims = dims
        if dims.lat_hist:
            lh_bytes = R * n_dc * 2 * (LH_BINS + 1) * 4
            (logger or logging.getLogger(LOGGER_NAME)).info(
                f"latency_hist: {R} replicas x {n_dc} DCs x 2 types x "
                f"({LH_BINS} bins + 1) x 4 B = {lh_bytes} bytes "
                f"({lh_bytes / 2**20:.1f} MiB), SLA {dims.lat_sla_s:g} s")
        if self.pop_series:
            ps_bytes = dims.ps_cap * (n_dc + 1) * len(SERIES_METRICS) * R * 8
            (logger or logging.getLogger(LOGGER_NAME)).info(
                f"pop_series: sample buffer {dims.ps_cap} ticks x {n_dc + 1} "
                f"rows x {len(SERIES_METRICS)} metrics x {R} replicas x 8 B = "
                f"{ps_bytes} bytes ({ps_bytes / 2**20:.1f} MiB)")
        sweep_table = sweep.table(shard, self.sweep_base) \
            if sweep is not None else None
        t = alloc_state(dims, scenario, dev, arrival_trace, sweep_table,
                        profile_table(scenario.n_ing, arrival_inf, arrival_trn)
                        if profile_on else None)
        if not self.trace_mode:
            # seed the initial arrival times on host (one inf + one trn per
            # ingress per replica), Philox-consistent with the device streams:
            # the kernel's first draws start at ctr = n_streams; host uses
            # ctr = stream index for the seed draws.  Under a sweep each
            # replica's draws use its own rate, amp and period.
            arr_np = self._seed_arrivals(arrival_inf, arrival_trn, seed, shard) \
                if sweep is None else seed_arrivals(
                    scenario.n_ing, self._sweep_procs(
                        arrival_inf, arrival_trn, sweep_table[0]), seed, shard)
            t["arr_next"].copy_(torch.as_tensor(arr_np, dtype=torch.float64))
        self.t = t
        self.arrival_inf, self.arrival_trn = arrival_inf, arrival_trn

        self._sim = self._mod.BatchedSimHip(
            t, engine_cfg(dims, scenario, arrival_inf, arrival_trn))
        self.meter = ThroughputMeter()
        if self.is_rl:
            self._rl_drv = rl_loop.RLDriver(
                t, self._sim, self._mod, dev, agent=self.rl,
                replay=self.replay, obs_dim=obs_dim, n_dc=n_dc, n_g=n_g,
                hid=RL_HID, serve_device=serve_device, mfma_serve=mfma_serve,
                deterministic=bool(rl_deterministic),
                use_graph=(world == 1 and rl_agent is None),
                batch=rl_batch, warmup=rl_warmup,
                train_interval=rl_train_interval,
                stats_interval=rl_stats_interval,
                target_updates_per_s=rl_target_updates_per_s,
                reserve_cus=rl_reserve_cus, world=world, logger=logger,
                end_time=self.end_time,
                events_per_launch=self.events_per_launch,
                drain_job_rows=self._drain_job_rows)

    # the RL driver's state, where callers have always found it
    @property
    def rl_updates(self) -> int:
        return self._rl_drv.rl_updates if self._rl_drv is not None else 0

    @property
    def _serve_device(self) -> bool:
        return self._rl_drv is not None and self._rl_drv.serve_device

    @property
    def _mfma_serve(self) -> bool:
        return self._rl_drv is not None and self._rl_drv.mfma_serve

    @_mfma_serve.setter
    def _mfma_serve(self, on: bool):
        self._rl_drv.mfma_serve = on

    def _seed_arrivals(self, arrival_inf, arrival_trn, seed, shard):
        """The seed draws of an engine whose replicas share one arrival pair
        (``seed_arrivals`` below)."""
        return seed_arrivals(self.sc.n_ing,
                             lambda r: (arrival_inf, arrival_trn), seed, shard)

    def _sweep_procs(self, arrival_inf, arrival_trn, sw_arr):
        """``procs_of_replica`` of a sweep: the base pair's modes with the
        replica's own rate, amp and period (``sw_arr`` [R, 2, 3])."""
        import dataclasses

        def procs(r):
            return tuple(dataclasses.replace(
                base, rate=float(sw_arr[r, jt, 0]), amp=float(sw_arr[r, jt, 1]),
                period=float(sw_arr[r, jt, 2]))
                for jt, base in enumerate((arrival_inf, arrival_trn)))
        return procs

    # ---------------- run ----------------
    def run(self, max_wall_s: Optional[float] = None):
        """Drive advance launches until every replica reaches end_time (or
        `max_wall_s` of wall clock passes — benchmarking aid).  One loop over
        one of three cycle bodies, each returning whether every replica is
        done: ``_cycle_plain`` for the non-RL algorithms, and for chsac_af
        ``RLDriver.cycle_sync`` (host serving, or data-parallel) or
        ``RLDriver.cycle_overlapped`` (single GPU, in-kernel serving)."""
        self.meter.start()
        tm = {"advance_s": 0.0, "serve_s": 0.0, "dp_sync_s": 0.0,
              "train_s": 0.0, "overlap_train_steps": 0, "launches": 0,
              "sync0_s": 0.0, "kernel_s": 0.0, "status_s": 0.0,
              "ingest_s": 0.0, "floor_s": 0.0, "refresh_s": 0.0}
        self.timing = tm
        cycle = self._cycle_plain if self._rl_drv is None \
            else self._rl_drv.start_run(tm)
        wall0 = time.perf_counter()
        while not cycle():
            if tm["launches"] > 1000000:
                raise RuntimeError("batched engine failed to converge")
            if max_wall_s and time.perf_counter() - wall0 > max_wall_s:
                break
        self.meter.count = int(self.t["ev_count"].sum().item())
        self.meter.stop()
        if self.log_replica >= 0 and self.out_dir is not None:
            self._write_logs()
        return self.stats()

    def _cycle_plain(self):
        """One launch of a non-RL run; returns True when every replica is
        done.  (``serve_s`` has always held the host work between launches.)"""
        with Lap(self.timing, "advance_s"):
            self._sim.advance(self.end_time, self.events_per_launch)
            self.timing["launches"] += 1
            st = read_status(self.t, ("err", "done", "n_jl"))
        with Lap(self.timing, "serve_s"):
            if st["err"] != 0 and self.sweep is not None:
                raise_on_group_err(self.t["err"], self.sweep, self.shard)
            raise_on_err(st["err"])
            self._drain_job_rows(st["n_jl"])
        return st["done"] == 1

    def _drain_job_rows(self, n_jl: int):
        """Chunk-wise drain of the device job-log buffer once it is half full,
        so unboundedly many job rows stream to the host (the reference streams
        rows to CSV unboundedly, simulator_paper_multi.py:814-823)."""
        t = self.t
        if n_jl < int(t["jl_rows"].shape[0]) // 2:
            return
        n = int(t["jl_count"].item())
        if n > 0:
            self._jl_chunks.append(t["jl_rows"][:n].cpu().numpy().copy())
            t["jl_count"].zero_()

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

    # ---------------- parameter sweep ----------------
    def _group_slice(self, group):
        """Local replica range ``[a, b)`` of sweep group ``group``."""
        if self.sweep is None:
            raise RuntimeError("engine was built without sweep=")
        return self.sweep.slice_of(int(group), self.shard)

    def _over_ranks(self, local, rebuild, merge):
        """One statistic over the whole ensemble.  ``local(gather)`` gives
        this rank's result when ``gather`` is false (no torch.distributed, or
        one rank: returned as is) and otherwise its flat f64 vector, of the
        same length on every rank; ``rebuild`` turns each rank's vector (a
        host tensor) back into a result and ``merge`` combines them, so every
        rank holds the global one."""
        from ..parallel.dist import allgather_series_stats, is_distributed
        gather = self.world > 1 and is_distributed()
        mine = local(gather)
        if not gather:
            return mine
        return merge([rebuild(p.cpu()) for p in allgather_series_stats(mine)])

    def sweep_stats(self):
        """Per-group statistics of the headline outcomes as a SweepStats
        (analysis/montecarlo.py): n / mean / M2 / min / max over each group's
        replicas of total energy, jobs, inference jobs, mean latency, mean
        inference latency, mean wait and events.  R x 7 numbers: numpy f64 on
        the host.  Under torch.distributed the per-rank statistics are
        merged, so every rank holds the global ones."""
        from ..analysis.montecarlo import (SWEEP_METRICS, SweepStats,
                                           merge_sweep_stats,
                                           sweep_replica_metrics)
        if self.sweep is None:
            raise RuntimeError("engine was built without sweep=")
        vals = sweep_replica_metrics({k: self.t[k].cpu().numpy() for k in (
            "energy_j", "jobs_done", "jobs_done_inf", "sum_lat",
            "sum_lat_inf", "sum_wait", "ev_count")})
        G = self.sweep.n_groups
        mine = SweepStats.from_values(
            vals, [self.sweep.slice_of(g, self.shard) for g in range(G)])
        return self._over_ranks(
            lambda gather: torch.from_numpy(mine.to_array().reshape(-1))
            if gather else mine,
            lambda p: SweepStats.from_array(
                p.numpy().reshape(G, len(SWEEP_METRICS), 5)),
            merge_sweep_stats)

    def population_series(self, group=None):
        """Per-tick statistics over the replica ensemble as a SeriesStats
        (analysis/montecarlo.py): n, mean, M2, min, max of every sampled
        metric per DC and fleet-wide, trimmed to the ticks at least one
        replica has reached.  Valid on an unfinished run (n counts the
        replicas that reached each tick).  Under torch.distributed the
        per-rank statistics are merged, so every rank holds the global
        series.  ``group=g`` (sweep engines): over that group's replicas on
        this rank only."""
        from ..analysis.montecarlo import SeriesStats, merge_series_stats
        ps = self.pop_samples()
        every = self.pop_series_every
        cap = int(ps["samples"].shape[0])
        n_row, K = self.sc.n_dc + 1, len(SERIES_METRICS)
        names = list(self.sc.dc_names) + [SERIES_FLEET]

        def wrap(flat_stats, time):
            return SeriesStats.from_tensor(
                flat_stats.view(len(time), n_row, K, 5), time,
                metrics=list(SERIES_METRICS), dc_names=names)

        if group is not None:
            a, b = self._group_slice(group)
            if b <= a:
                raise ValueError(f"this rank holds no replica of group {group}")
            ticks = ps["ticks"][a:b].contiguous()
            T = min(cap, int(ticks.max().item()) // every)
            # replica-minor buffer: the group's columns, packed
            smp = ps["samples"][:T, :, :, a:b].contiguous()
            raw = self._mod.reduce_series(
                smp.view(T, n_row * K, b - a), ticks, every)
            return wrap(raw.cpu(), ps["time"][:T].cpu()).trimmed()

        def local(gather):
            # ranks must agree on the shape they gather: the full buffer then
            T = cap if gather else \
                min(cap, int(ps["ticks"].max().item()) // every)
            raw = self._mod.reduce_series(
                ps["samples"][:T].view(T, n_row * K, self.R), ps["ticks"],
                every)
            if gather:
                return torch.cat([raw.reshape(-1), ps["time"][:T]])
            return wrap(raw.cpu(), ps["time"][:T].cpu())

        return self._over_ranks(local, lambda p: wrap(p[:-cap], p[-cap:]),
                                merge_series_stats).trimmed()

    # ---------------- latency histograms ----------------
    def latency_hist(self):
        """Raw device views of the per-replica latency histograms: ``hist``
        [R, n_dc, 2, 256] (bins: analysis/montecarlo.latency_bin_edges),
        ``over`` [R, n_dc, 2] (finishes with sojourn > ``sla_s``)."""
        if not self.dims.lat_hist:
            raise RuntimeError("engine was built without latency_hist=True")
        return {"hist": self.t["lh_hist"], "over": self.t["lh_over"],
                "sla_s": self.dims.lat_sla_s}

    def latency_distribution(self, quantiles=(0.5, 0.9, 0.99, 0.999),
                             group=None):
        """Latency quantiles, SLA-miss fraction and job count per (DC, job
        type) and fleet-wide as a LatencyStats (analysis/montecarlo.py): the
        histogram pooled over the replicas, and n / mean / M2 / min / max of
        every per-replica figure over the replicas that have one.  Valid on an
        unfinished run.  Under torch.distributed the per-rank results are
        merged, so every rank holds the global one.  ``group=g`` (sweep
        engines): over that group's replicas on this rank only."""
        from ..analysis.montecarlo import LatencyStats, merge_latency_stats
        lh = self.latency_hist()
        qs = [float(q) for q in quantiles]
        hist, over = lh["hist"], lh["over"]
        if group is not None:
            a, b = self._group_slice(group)
            if b <= a:
                raise ValueError(f"this rank holds no replica of group {group}")
            hist, over = hist[a:b], over[a:b]   # replica-major: contiguous
        pop, _, stats = self._mod.latency_reduce(
            hist, over, torch.tensor(qs, dtype=torch.float64))
        names = list(self.sc.dc_names) + [SERIES_FLEET]
        n_row, K = len(names), len(qs) + 2
        mine = LatencyStats.from_tensor(
            pop.cpu().view(n_row, 2, LH_BINS), stats.cpu().view(n_row, 2, K, 5),
            quantiles=qs, dc_names=names, sla_s=lh["sla_s"])
        if group is not None:
            return mine
        # the histogram travels as f64 with the statistics: exact below 2^53
        return self._over_ranks(
            lambda gather: torch.from_numpy(mine.to_flat()) if gather
            else mine,
            lambda p: LatencyStats.from_flat(p.numpy(), qs, names,
                                             lh["sla_s"]),
            merge_latency_stats)

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
        # a sweep's parameters are state: a checkpoint of another sweep (or
        # of other base values) would silently change this engine's points
        for k in ("sw_arr", "sw_cap", "arr_prof"):
            if k in self.t and k in st["tensors"] and \
                    tuple(st["tensors"][k].shape) == tuple(self.t[k].shape) \
                    and not torch.equal(st["tensors"][k].to(self.t[k].dtype),
                                        self.t[k].cpu()):
                raise ValueError(
                    f"checkpoint tensor {k!r} differs from this engine's own "
                    + ("rate profile" if k == "arr_prof" else
                       "sweep: it was saved by an engine with other "
                       "parameter points"))
        load_tensors(self.t, st["tensors"])
        if self._rl_drv is not None:
            self._rl_drv.rl_updates = st.get("rl_updates", 0)
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
