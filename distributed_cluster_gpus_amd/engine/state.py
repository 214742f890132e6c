"""Device state of the batched replica engine: sizes, allocation, config.

``engine_dims`` computes every size and option once (EngineDims);
``alloc_state`` allocates the replica-major SoA state from it, on any device
("cpu" included, which is how the host <-> device contract is tested without a
GPU); ``engine_cfg`` is the scalar config dict of ``BatchedSimHip``.  The
tensor names are the pointer fields of EngineDesc
(ops/csrc/hip/engine_desc.hpp); the extension checks dtype, extent, contiguity
and device of each when it binds them (engine_bind.hpp).

Three allocations are placeholders, because only one configuration's kernel
dereferences the field: ``snap_f`` is (1, 1) unless the algo is cap_greedy,
``b_n`` / ``b_s`` have a leading dim of 1 unless it is bandit, ``p99_sorted``
/ ``p99_ring`` are (1, 1, 1) without exact_p99.  The extension neither binds
nor checks those (``contract()`` lists them as not required).

The arrival ring (``arr_ring``, ``arr_head``, ``arr_count``, the generator's
frontier ``gen_arr_next`` / ``gen_ctr`` and the ``arr_more`` flag;
ops/csrc/hip/arrival_ring.hpp) exists only where arrivals are pre-generated:
every algo but chsac_af, outside trace mode, unless ``arrival_pregen=False``.
It is ordinary state: a checkpoint saves and restores it with the rest.

The latency histograms (``lh_hist``, ``lh_over``; ops/csrc/hip/lat_hist.hpp)
exist only when asked for (``latency_hist=True``); their presence is what
selects the recording kernels.  Ordinary state as well.

The rate-profile table (``arr_prof``; ops/csrc/hip/arrival_ring.hpp) exists
only when a job type's arrival mode is 'profile'; its presence selects the
PROF arrival-ring generators.  Constant over a run, saved and restored with
the rest.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ..models.scenario import PAYLOAD_GB, Scenario

ALGO_IDS = {"default_policy": 0, "cap_uniform": 1, "cap_greedy": 2,
            "joint_nf": 3, "bandit": 4, "carbon_cost": 5, "eco_route": 6,
            "debug": 7, "chsac_af": 8}
ECO_IDS = {"energy": 0, "carbon": 1, "cost": 2}
MODE_IDS = {"poisson": 0, "sinusoid": 1, "off": 2, "profile": 3}
PROF_SEG = 64      # most segments of a rate profile (PROF_MAX_SEG)
PROF_W = 2 * PROF_SEG + 2   # f64 per arr_prof row: K, m[64], cum[65] (PROF_W)
INF = 1e300
# population-series metrics per DC, in sample-buffer order (PS_K in
# ops/csrc/hip/pop_series.hpp)
SERIES_METRICS = ("freq", "busy", "running", "q_inf", "q_trn", "power_w",
                  "energy_j")
RL_HID = 256       # served actor's hidden width (RL_MAX_HID)
P99_WIN = 2048     # exact-p99 sliding window (the reference's 2048 sojourns)
ARR_CAP = 4096     # arrival-ring records per replica (32 B each): one
                   # advance() call of up to this many events is one sub-step
LH_BINS = 256      # latency-histogram bins (ops/csrc/hip/lat_bins.hpp)


@dataclass(frozen=True)
class EngineDims:
    """Every size and option the state allocation and the config dict need."""
    algo: str
    n_rep: int
    n_dc: int
    n_ing: int
    n_freq: int
    total_slots: int
    tcap: int
    qcap: int
    end_time: float
    log_interval: float
    log_replica: int            # -1 = off
    cl_cap: int
    jl_cap: int
    ps_every: int               # population series: 0 = off
    ps_cap: int
    trace_mode: bool
    trace_cap: int
    # policy / run parameters
    power_cap: float
    eco_obj: int
    fp32_score: int
    num_fixed: int
    fixed_freq: float
    seed: int
    rep_id_offset: int
    sla_p99_ms: float
    # CHSAC-AF (zero / off for every other algo)
    obs_dim: int
    tr_cap: int
    pp_cap: int
    elastic: int
    exact_p99: int
    serve_device: int
    weights_numel: int          # flat actor-weights buffer; 1 = placeholder
    rl_det: int
    tr_limit: int
    arr_cap: int = 0            # arrival ring: records per replica; 0 = off
    lat_hist: bool = False      # per-replica latency histograms
    lat_sla_s: float = 0.5      # ... and the sojourn their SLA-miss count uses
    sweep: bool = False         # parameter sweep (engine/sweep.py): sw_* exist
    sweep_cap: bool = False     # ... and it has a power_cap axis
    profile: bool = False       # a job type is in 'profile' mode: arr_prof

    @property
    def is_rl(self) -> bool:
        return self.algo == "chsac_af"

    @property
    def n_streams(self) -> int:
        return self.n_ing * 2


def policy_weights_numel(obs_dim: int, n_dc: int, n_g: int,
                         hid: int = RL_HID) -> int:
    """Seven-layer flat layout documented at EngineDesc::pw."""
    H = hid
    return (obs_dim * H + H) + 2 * (H * H + H) + (H * H + H) + \
        (H * n_dc + n_dc) + (H * H + H) + (H * n_g + n_g)


def engine_dims(scenario: Scenario, *, algo: str, n_rep: int,
                duration: float = 3600.0, log_interval: float = 10.0,
                tcap: int = 64, qcap: int = 24576,
                events_per_launch: int = 50000, log_replica: int = -1,
                pop_series_every: int = 0, arrival_trace=None,
                power_cap: float = 0.0, eco_objective: str = "energy",
                fp32_coeff_eval: bool = False, num_fixed_gpus: int = 1,
                fixed_freq: Optional[float] = None, seed: int = 42,
                rep_id_offset: int = 0, sla_p99_ms: float = 500.0,
                tr_cap: int = 262144, elastic_scaling: bool = False,
                rl_exact_p99: bool = False, serve_device: bool = False,
                weights_buffer: bool = False, rl_deterministic: bool = False,
                rl_tr_limit: Optional[int] = None,
                rl_train_interval: int = 256,
                arrival_pregen: bool = True,
                arr_cap: int = ARR_CAP, latency_hist: bool = False,
                latency_sla_s: Optional[float] = None,
                sweep=None, arrivals=None) -> EngineDims:
    """``n_rep`` is this rank's replica count; ``serve_device`` /
    ``weights_buffer`` say whether the kernel serves the policy itself and
    whether the flat actor-weights buffer is needed at all (it also feeds the
    host path's matrix-core forward).  ``arrival_pregen`` asks for the arrival
    ring of ``arr_cap`` records (a power of two) per replica; chsac_af and
    trace mode never have one.  ``latency_hist`` asks for the per-replica
    latency histograms; ``latency_sla_s`` (default ``sla_p99_ms / 1000``) is
    the sojourn above which a finish counts as an SLA miss.  ``sweep`` (a
    ``Sweep``) records that a parameter sweep is on; it needs the ring.
    ``arrivals`` (the ``(inference, training)`` pair) records whether a job
    type is in 'profile' mode, which needs the ring as well."""
    is_rl = algo == "chsac_af"
    n_dc = scenario.n_dc
    end_time, log_interval = float(duration), float(log_interval)
    n_ticks = int(math.ceil(end_time / log_interval))
    # Job rows are drained chunk-wise between launches, so jl_cap bounds only
    # ONE launch's production: the logging replica emits at most one job row
    # per event, hence events_per_launch rows per launch.
    logs = log_replica >= 0
    obs_dim = 1 + 6 * n_dc
    n_g = int(scenario.policy.max_gpus_per_job)
    tr_cap = int(tr_cap) if is_rl else 0
    # default yield point: long enough that the overlapped loop can sustain
    # back-to-back train-graph replays under the advance window, short enough
    # to bound policy staleness to one cycle of transitions
    tr_limit = int(rl_tr_limit) if rl_tr_limit is not None else \
        min(tr_cap // 2, int(rl_train_interval) * 256)
    pregen = bool(arrival_pregen) and not is_rl and arrival_trace is None
    if pregen and (int(arr_cap) < 1 or int(arr_cap) & (int(arr_cap) - 1)):
        raise ValueError(f"arr_cap must be a power of two, got {arr_cap}")
    if sweep is not None and not pregen:
        raise ValueError("a sweep lives in the arrival-ring generator: it "
                         "needs arrival_pregen, no arrival_trace and an algo "
                         "other than chsac_af")
    if sweep is not None and sweep.has_power_cap and algo != "cap_greedy":
        raise ValueError("a power_cap sweep axis needs algo='cap_greedy', "
                         f"got {algo!r}")
    profile = arrivals is not None and any(
        a.mode == "profile" for a in arrivals)
    if profile and not pregen:
        raise ValueError("arrival mode 'profile' lives in the arrival-ring "
                         "generator: it needs arrival_pregen, no "
                         "arrival_trace and an algo other than chsac_af")
    return EngineDims(
        algo=algo, n_rep=int(n_rep), n_dc=n_dc, n_ing=scenario.n_ing,
        n_freq=scenario.n_freq,
        total_slots=int(scenario.total_gpus.sum()), tcap=int(tcap),
        qcap=int(qcap), end_time=end_time, log_interval=log_interval,
        log_replica=int(log_replica),
        cl_cap=(n_dc * (n_ticks + 2) + 64) if logs else 1,
        jl_cap=max(65536, 2 * int(events_per_launch)) if logs else 1,
        ps_every=int(pop_series_every),
        ps_cap=(n_ticks // int(pop_series_every) + 2) if pop_series_every
        else 0,
        trace_mode=arrival_trace is not None,
        trace_cap=int(np.asarray(arrival_trace[0]).shape[2])
        if arrival_trace is not None else 0,
        power_cap=float(power_cap), eco_obj=ECO_IDS[eco_objective],
        fp32_score=int(bool(fp32_coeff_eval)), num_fixed=int(num_fixed_gpus),
        fixed_freq=float(fixed_freq) if fixed_freq else 0.0,
        seed=int(seed), rep_id_offset=int(rep_id_offset),
        sla_p99_ms=float(sla_p99_ms),
        obs_dim=obs_dim, tr_cap=tr_cap,
        # elastic-scaling preempted-job pool: a DC can run up to total_gpus
        # concurrent 1-GPU training jobs, all preemptible
        pp_cap=int(scenario.total_gpus.max()) if is_rl else 0,
        elastic=int(bool(elastic_scaling) and is_rl),
        exact_p99=int(bool(rl_exact_p99) and is_rl),
        serve_device=int(bool(serve_device) and is_rl),
        weights_numel=policy_weights_numel(obs_dim, n_dc, n_g)
        if (is_rl and (serve_device or weights_buffer)) else 1,
        rl_det=int(bool(rl_deterministic) and is_rl),
        tr_limit=tr_limit if is_rl else 0,
        arr_cap=int(arr_cap) if pregen else 0,
        lat_hist=bool(latency_hist),
        lat_sla_s=float(latency_sla_s) if latency_sla_s is not None
        else float(sla_p99_ms) / 1000.0,
        sweep=sweep is not None,
        sweep_cap=sweep is not None and sweep.has_power_cap,
        profile=profile)


def validate_profile_engine(arrival_inf, arrival_trn, n_ing, *, algo,
                            subwave=64, arrival_pregen=True,
                            arrival_trace=None) -> bool:
    """Whether a job type is in 'profile' mode; ValueError, with the reason,
    where such an engine cannot be built.  Plain Python: runs before anything
    touches a GPU."""
    from ..models.arrivals import check_profile
    named = (("inference", arrival_inf), ("training", arrival_trn))
    on = [(n, a) for n, a in named if a.mode == "profile"]
    for name, a in on:
        try:
            rows = check_profile(a.profile).shape[0]
        except ValueError as e:
            raise ValueError(f"{name} arrivals: {e}") from None
        if rows not in (1, int(n_ing)):
            raise ValueError(
                f"{name} arrivals: profile has {rows} rows; it needs 1 "
                f"(shared) or n_ing = {n_ing}")
        if not (math.isfinite(a.period) and a.period > 0):
            raise ValueError(f"{name} arrivals: profile period = {a.period} "
                             "must be > 0")
        if not (math.isfinite(a.rate) and a.rate >= 0):
            raise ValueError(f"{name} arrivals: profile rate = {a.rate} "
                             "must be finite and >= 0")
    if not on:
        return False
    why = "arrival mode 'profile' lives in the arrival-ring generator"
    if algo == "chsac_af":
        raise ValueError(f"{why}; algo='chsac_af' draws its arrivals inside "
                         "the advance kernel")
    if int(subwave) != 64:
        raise ValueError(f"{why}; the 8-lane build (subwave={subwave}) has "
                         "none")
    if not arrival_pregen:
        raise ValueError(f"{why}; arrival_pregen=False draws inside the "
                         "advance kernel")
    if arrival_trace is not None:
        raise ValueError(f"{why}; arrival_trace replays recorded arrivals "
                         "instead of drawing any")
    return True


def profile_table(n_ing, arrival_inf, arrival_trn) -> np.ndarray:
    """``arr_prof``: [n_streams, PROF_W] f64, row ``ing * 2 + jtype`` = (K,
    m[0..K-1] padded to 64, cum[0..K] padded to 65); a job type that is not
    in profile mode has rows of zeros (K = 0), which nobody reads."""
    from ..models.arrivals import profile_tables
    tab = np.zeros((n_ing * 2, PROF_W))
    for jt, a in enumerate((arrival_inf, arrival_trn)):
        if a.mode != "profile":
            continue
        for i, row in enumerate(a.profile_rows(n_ing)):
            m, cum = profile_tables(row)
            K = len(m)
            tab[i * 2 + jt, 0] = K
            tab[i * 2 + jt, 1:1 + K] = m
            tab[i * 2 + jt, 1 + PROF_SEG:2 + PROF_SEG + K] = cum
    return tab


def alloc_state(dims: EngineDims, scenario: Scenario, device,
                arrival_trace=None, sweep_table=None, prof_table=None) -> dict:
    """The engine's tensors by EngineDesc field name, in their initial state.
    ``arr_next`` holds the trace's first arrivals in trace mode and +inf
    otherwise (the caller seeds it); ``rng_ctr`` starts past the one counter
    block per stream that seeding consumes.  ``sweep_table`` is the ``(arr,
    cap)`` pair of ``Sweep.table`` for this rank's replicas, required exactly
    when ``dims.sweep``; ``prof_table`` is ``profile_table``'s, required
    exactly when ``dims.profile``."""
    d = dims
    dev = torch.device(device)
    R, n_dc, n_freq, NS = d.n_rep, d.n_dc, d.n_freq, d.n_streams
    total_slots, tcap, qcap = d.total_slots, d.tcap, d.qcap
    f64 = dict(dtype=torch.float64, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    i16 = dict(dtype=torch.int16, device=dev)
    i8 = dict(dtype=torch.int8, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)

    def T(arr, **kw):
        # copy=True: on the CPU the state must not alias the caller's arrays
        return torch.as_tensor(np.ascontiguousarray(arr), **kw).to(
            dev, copy=True)

    slot_off = np.zeros(n_dc + 1, np.int32)
    slot_off[1:] = np.cumsum(scenario.total_gpus)
    slot_dc = np.zeros(total_slots, np.int32)
    for k in range(n_dc):
        slot_dc[slot_off[k]:slot_off[k + 1]] = k

    t = {}
    # scenario constants
    t["freq_levels"] = T(scenario.freq_levels, dtype=torch.float64)
    t["pc"] = T(scenario.power_coeffs.reshape(-1), dtype=torch.float64)
    t["lc"] = T(scenario.latency_coeffs.reshape(-1), dtype=torch.float64)
    t["wan_lat"] = T(np.asarray(scenario.wan_latency_s).reshape(-1), dtype=torch.float64)
    t["wan_bw"] = T(np.asarray(scenario.wan_bottleneck_gbps).reshape(-1), dtype=torch.float64)
    t["carbon"] = T(scenario.carbon_vec(), dtype=torch.float64)
    t["price24"] = T(scenario.price_vec24(), dtype=torch.float64)
    t["total_gpus"] = T(scenario.total_gpus, dtype=torch.int32)
    t["p_idle"] = T(scenario.p_idle, dtype=torch.float64)
    t["p_sleep"] = T(scenario.p_sleep, dtype=torch.float64)
    t["p_peak"] = T([scenario.gpu_specs[n].p_peak for n in scenario.dc_names],
                    dtype=torch.float64)
    t["pow_alpha"] = T([scenario.gpu_specs[n].alpha for n in scenario.dc_names],
                       dtype=torch.float64)
    t["power_gating"] = T(scenario.power_gating.astype(np.int32), dtype=torch.int32)
    t["default_freq"] = T(scenario.default_freq, dtype=torch.float64)
    t["slot_off"] = T(slot_off, dtype=torch.int32)
    t["slot_dc"] = T(slot_dc, dtype=torch.int32)
    # per-replica state
    t["now"] = torch.full((R,), -1.0, **f64)
    t["next_log"] = torch.full((R,), d.log_interval, **f64)
    t["rng_ctr"] = torch.full((R,), NS, **i64)
    t["jid_ctr"] = torch.zeros(R, **i32)
    t["done"] = torch.zeros(R, **i32)
    t["err"] = torch.zeros(R, **i32)
    t["arr_next"] = torch.full((R, NS), INF, **f64)
    t["busy"] = torch.zeros((R, n_dc), **i32)
    t["cur_freq"] = torch.empty((R, n_dc), **f64)
    t["cur_freq"][:] = torch.as_tensor(scenario.default_freq, dtype=torch.float64,
                                       device=dev)
    t["energy_j"] = torch.zeros((R, n_dc), **f64)
    t["util_time"] = torch.zeros((R, n_dc), **f64)
    t["util_begin"] = torch.full((R, n_dc), -1.0, **f64)
    t["acc_unit"] = torch.zeros((R, n_dc), **f64)
    t["p_active"] = torch.zeros((R, n_dc), **f64)
    t["sum_tpt"] = torch.zeros((R, n_dc), **f64)
    t["n_running"] = torch.zeros((R, n_dc), **i32)
    t["dc_min_finish"] = torch.full((R, n_dc), INF, **f64)
    t["dc_min_slot"] = torch.full((R, n_dc), -1, **i32)
    t["s_finish"] = torch.full((R, total_slots), INF, **f64)
    # packed cold slot payload (SRec, 64 B — start/lastupd/size/fused/
    # done f64, netlat f32, jid/seq i32, ing/pcount/RL-trace bytes);
    # one cache line per job start/finish instead of 10+ SoA touches
    t["s_rec"] = torch.zeros((R, total_slots, 8), **f64)
    t["seq_ctr"] = torch.zeros(R, **i32)
    t["s_gpus"] = torch.zeros((R, total_slots), **i16)
    t["s_jtype"] = torch.zeros((R, total_slots), **i8)
    t["x_time"] = torch.full((R, tcap), INF, **f64)
    # packed transfer payload (XRec, 32 B)
    t["x_rec"] = torch.zeros((R, tcap, 4), **f64)
    t["q_head"] = torch.zeros((R, n_dc, 2), **i32)
    t["q_len"] = torch.zeros((R, n_dc, 2), **i32)
    # per-entry (size, enqueue-time) f64 pair — one line per push/pop
    t["q_pay"] = torch.zeros((R, n_dc, 2, qcap, 2), **f64)
    # cap_greedy pass-snapshot scratch (frozen task frequencies)
    t["snap_f"] = torch.zeros(
        (R, total_slots) if d.algo == "cap_greedy" else (1, 1), **f64)
    # queue aux fields (net latency / jid / ingress) are only consumed by
    # the logging replica's job rows -> single-replica allocation
    t["q_netlat"] = torch.zeros((n_dc, 2, qcap), **f32)
    t["q_jid"] = torch.zeros((n_dc, 2, qcap), **i32)
    t["q_ing"] = torch.zeros((n_dc, 2, qcap), **i8)
    nb = R if d.algo == "bandit" else 1
    t["b_n"] = torch.zeros((nb, n_dc, 2, n_freq), **i32)
    t["b_s"] = torch.zeros((nb, n_dc, 2, n_freq), **f64)
    t["b_t"] = torch.zeros(R, **i64)
    t["ev_count"] = torch.zeros(R, **i64)
    t["jobs_done"] = torch.zeros(R, **i64)
    t["jobs_done_inf"] = torch.zeros(R, **i64)
    t["sum_lat"] = torch.zeros(R, **f64)
    t["sum_lat_inf"] = torch.zeros(R, **f64)
    t["sum_wait"] = torch.zeros(R, **f64)
    # logging buffers (one designated replica)
    t["cl_count"] = torch.zeros(1, **i32)
    t["cl_rows"] = torch.zeros((d.cl_cap, 15), **f64)
    t["jl_count"] = torch.zeros(1, **i32)
    t["jl_rows"] = torch.zeros((d.jl_cap, 11), **f64)

    # population time series (opt-in): every replica snapshots PS_K metrics
    # per DC plus one fleet row at every ps_every-th log tick.  Launches are
    # bounded by events, so replicas drift apart: the buffer covers the WHOLE
    # run and is indexed by the per-replica tick counter ps_tick.
    if d.ps_every:
        t["ps_samples"] = torch.zeros(
            (d.ps_cap, n_dc + 1, len(SERIES_METRICS), R), **f64)
        t["ps_time"] = torch.zeros(d.ps_cap, **f64)
        t["ps_tick"] = torch.zeros(R, **i32)

    # arrival ring: records (ARec, 32 B) the generator appends and the
    # advance kernel consumes, and the generator's frontier.  The frontier is
    # re-read from arr_next / rng_ctr whenever the ring is empty, so it needs
    # no seeding here.
    if d.arr_cap:
        t["arr_ring"] = torch.zeros((R, d.arr_cap, 4), **f64)
        t["arr_head"] = torch.zeros(R, **i32)
        t["arr_count"] = torch.zeros(R, **i32)
        t["gen_arr_next"] = torch.full((R, NS), INF, **f64)
        t["gen_ctr"] = torch.zeros(R, **i64)
        t["arr_more"] = torch.zeros(1, **i32)

    # latency histograms (opt-in): every replica counts each job finish by
    # (DC, job type, sojourn bin), and the finishes above the SLA
    if d.lat_hist:
        t["lh_hist"] = torch.zeros((R, n_dc, 2, LH_BINS), **i32)
        t["lh_over"] = torch.zeros((R, n_dc, 2), **i32)

    # parameter sweep (opt-in): every replica's own arrival parameters and
    # power cap, constant over the run.  sw_arr is read by the arrival-ring
    # generator, sw_cap by the cap_greedy kernel where the sweep has a
    # power_cap axis (elsewhere it holds the base cap and nobody reads it)
    if d.sweep != (sweep_table is not None):
        raise ValueError("alloc_state: sweep_table goes with dims.sweep")
    if d.sweep:
        sw_arr, sw_cap = (np.asarray(x, np.float64) for x in sweep_table)
        if sw_arr.shape != (R, 2, 3) or sw_cap.shape != (R,):
            raise ValueError(
                f"sweep table is {sw_arr.shape} / {sw_cap.shape}, this rank's "
                f"{R} replicas need {(R, 2, 3)} / {(R,)}")
        t["sw_arr"] = T(sw_arr, dtype=torch.float64)
        t["sw_cap"] = T(sw_cap, dtype=torch.float64)

    # per-stream rate profiles (opt-in): read by the PROF arrival-ring
    # generators, written by nobody on the device
    if d.profile != (prof_table is not None):
        raise ValueError("alloc_state: prof_table goes with dims.profile")
    if d.profile:
        tab = np.asarray(prof_table, np.float64)
        if tab.shape != (NS, PROF_W):
            raise ValueError(f"profile table is {tab.shape}, {NS} streams "
                             f"need {(NS, PROF_W)}")
        t["arr_prof"] = T(tab, dtype=torch.float64)

    # arrival-trace replay mode (exact single-replica parity testing):
    # arrivals come from a recorded (time, size) FIFO per stream
    if d.trace_mode:
        # (times, sizes[, routed_dcs]) — routed_dcs entries of -1 let the
        # algorithm's own routing run (eco_route); >=0 replays the
        # recorded DC choice (exact-parity for random-routing algos)
        tt, ts = arrival_trace[0], arrival_trace[1]
        td = arrival_trace[2] if len(arrival_trace) > 2 else \
            np.full(np.asarray(tt).shape, -1, np.int8)
        tt = np.asarray(tt, np.float64)
        ts = np.asarray(ts, np.float64)
        td = np.asarray(td, np.int8)
        assert tt.shape == (R, NS, d.trace_cap), tt.shape
        t["trace_time"] = T(tt)
        t["trace_size"] = T(ts)
        t["trace_dc"] = T(td)
        t["trace_pos"] = torch.zeros((R, NS), **i32)
        t["arr_next"].copy_(t["trace_time"][:, :, 0])

    if d.is_rl:
        obs_dim, pp_cap, tr_cap = d.obs_dim, d.pp_cap, d.tr_cap
        t["req_flag"] = torch.zeros(R, **i32)
        t["req_obs"] = torch.zeros((R, obs_dim), **f32)
        t["req_mdc"] = torch.zeros(R, **i32)
        t["req_mg"] = torch.zeros(R, **i32)
        t["resp_dc"] = torch.zeros(R, **i32)
        t["resp_g"] = torch.zeros(R, **i32)
        t["pend_kind"] = torch.zeros(R, **i32)
        t["pend_size"] = torch.zeros(R, **f64)
        t["pend_netlat"] = torch.zeros(R, **f32)
        t["pend_jid"] = torch.zeros(R, **i32)
        t["pend_ing"] = torch.zeros(R, **i32)
        t["pend_jt"] = torch.zeros(R, **i32)
        t["pend_dc"] = torch.zeros(R, **i32)
        t["pend_from_inf"] = torch.zeros(R, **i32)
        t["pend_enq"] = torch.zeros(R, **f64)
        # per-job RL obs traces; action/mask bytes live in s_rec/x_rec
        t["slot_s0"] = torch.zeros((R, total_slots, obs_dim), **f32)
        t["x_s0"] = torch.zeros((R, tcap, obs_dim), **f32)
        # elastic-scaling preempted-job pool
        t["pp_count"] = torch.zeros(R, **i32)
        t["pp_cursor"] = torch.zeros(R, **i32)
        t["pp_size"] = torch.zeros((R, pp_cap), **f64)
        t["pp_done"] = torch.zeros((R, pp_cap), **f64)
        t["pp_start"] = torch.zeros((R, pp_cap), **f64)
        t["pp_netlat"] = torch.zeros((R, pp_cap), **f32)
        t["pp_jid"] = torch.zeros((R, pp_cap), **i32)
        t["pp_ing"] = torch.zeros((R, pp_cap), **u8)
        t["pp_dc"] = torch.zeros((R, pp_cap), **u8)
        t["pp_pcount"] = torch.zeros((R, pp_cap), **u8)
        t["pp_s0"] = torch.zeros((R, pp_cap, obs_dim), **f32)
        t["pp_adc"] = torch.zeros((R, pp_cap), **u8)
        t["pp_ag"] = torch.zeros((R, pp_cap), **u8)
        t["pp_nrew"] = torch.zeros((R, pp_cap), **u8)
        t["pp_has_rl"] = torch.zeros((R, pp_cap), **u8)
        t["lat_hist"] = torch.zeros((R, 2, 64), **i32)
        t["lat_count"] = torch.zeros((R, 2), **i64)
        t["lat_sum"] = torch.zeros((R, 2), **f64)
        # exact sliding-window p99 (parity mode): sorted window + ring
        # reproducing the reference's np.percentile over 2048 sojourns
        p99_shape = (R, 2, P99_WIN) if d.exact_p99 else (1, 1, 1)
        t["p99_sorted"] = torch.zeros(p99_shape, **f64)
        t["p99_ring"] = torch.zeros(p99_shape, **f64)
        # transition ring (global across replicas; drained between launches)
        t["tr_count"] = torch.zeros(1, **i32)
        t["tr_s0"] = torch.zeros((tr_cap, obs_dim), **f32)
        t["tr_s1"] = torch.zeros((tr_cap, obs_dim), **f32)
        t["tr_adc"] = torch.zeros(tr_cap, **u8)
        t["tr_ag"] = torch.zeros(tr_cap, **u8)
        t["tr_r"] = torch.zeros(tr_cap, **f32)
        t["tr_costs"] = torch.zeros((tr_cap, 3), **f32)
        t["tr_mdc"] = torch.zeros(tr_cap, **u8)
        t["tr_mg"] = torch.zeros(tr_cap, **u8)
        # flat fp32 actor-weights buffer for in-kernel serving and the host
        # path's matrix-core forward (layout: EngineDesc::pw)
        t["policy_weights"] = torch.zeros(d.weights_numel, **f32)
    return t


def load_tensors(state: dict, saved: dict) -> None:
    """Copy a checkpoint's tensors into ``state``.  The two must match key
    for key and each tensor in shape and dtype (``copy_`` alone would
    broadcast a placeholder into a full-size tensor and skip a missing key);
    raises ValueError naming the first mismatch before anything is copied."""
    for k in state:
        if k not in saved:
            raise ValueError(f"checkpoint lacks tensor {k!r}")
    for k, v in saved.items():
        if k not in state:
            raise ValueError(f"checkpoint tensor {k!r} is not part of this "
                             "engine's state")
        have = state[k]
        if tuple(v.shape) != tuple(have.shape) or v.dtype != have.dtype:
            raise ValueError(
                f"checkpoint tensor {k!r} is {v.dtype} {tuple(v.shape)}, "
                f"this engine's is {have.dtype} {tuple(have.shape)}")
    for k, v in saved.items():
        state[k].copy_(v.to(state[k].device))


def engine_cfg(dims: EngineDims, scenario: Scenario, arrival_inf,
               arrival_trn) -> dict:
    """Scalar config of ``BatchedSimHip(tensors, cfg)``."""
    d, pol = dims, scenario.policy
    return {
        "n_rep": d.n_rep, "n_dc": d.n_dc, "n_ing": d.n_ing,
        "n_freq": d.n_freq, "total_slots": d.total_slots, "tcap": d.tcap,
        "qcap": d.qcap, "end_time": d.end_time,
        "log_interval": d.log_interval, "algo": ALGO_IDS[d.algo],
        "max_gpj": int(pol.max_gpus_per_job),
        "inf_priority": int(pol.inf_priority),
        "scale_out_low": int(pol.train_scale_out_low_freq),
        "energy_aware": int(pol.name == "energy_aware"),
        "dvfs_low": float(pol.dvfs_low), "dvfs_high": float(pol.dvfs_high),
        "power_cap": d.power_cap, "eco_obj": d.eco_obj,
        "fp32_score": d.fp32_score, "num_fixed": d.num_fixed,
        "fixed_freq": d.fixed_freq,
        "payload_inf_gb": PAYLOAD_GB[0], "payload_trn_gb": PAYLOAD_GB[1],
        "arr_mode": [MODE_IDS[arrival_inf.mode], MODE_IDS[arrival_trn.mode]],
        "arr_rate": [float(arrival_inf.rate), float(arrival_trn.rate)],
        "arr_amp": [float(arrival_inf.amp), float(arrival_trn.amp)],
        "arr_period": [float(arrival_inf.period), float(arrival_trn.period)],
        "seed": d.seed, "rep_id_offset": d.rep_id_offset,
        "log_replica": d.log_replica, "cl_cap": d.cl_cap, "jl_cap": d.jl_cap,
        "obs_dim": d.obs_dim, "sla_p99_ms": d.sla_p99_ms, "tr_cap": d.tr_cap,
        "elastic": d.elastic, "pp_cap": d.pp_cap,
        "trace_mode": int(d.trace_mode), "trace_cap": d.trace_cap,
        "serve_device": d.serve_device, "rl_hid": RL_HID, "rl_det": d.rl_det,
        "tr_limit": d.tr_limit, "exact_p99": d.exact_p99,
        "p99_win": P99_WIN, "pop_series_every": d.ps_every,
        "arr_cap": d.arr_cap, "lat_sla_s": d.lat_sla_s,
        "sweep_cap": int(d.sweep_cap),
    }
