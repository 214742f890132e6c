"""Host side of CHSAC-AF in the loop: everything BatchedEngine needs to drive
chsac_af around the advance kernel, and nothing a non-RL run touches.

* ``ServingWeights`` — the flat actor-weights buffer the advance kernel and
  ``rl_forward_mfma`` read (layout: EngineDesc::pw).
* ``pace_train`` — the one rule that turns the transition backlog into SAC
  train steps.
* ``RLDriver`` — serve / ingest / train and the two cycle bodies (synchronous,
  single-rank or data-parallel; overlapped) that ``BatchedEngine.run()`` loops
  over.  It works on any device: the CPU tests drive it with a stub sim.
"""
import time
import warnings

import torch

from ..parallel.dist import dp_sync_step, is_distributed
from ..rl.agent import CHSACAgentConfig, make_agent
from ..rl.graphed import GraphedSACStep
from ..rl.masking import sample_categorical
from ..rl.replay import ReplayRing
from ..utils.timers import Lap
from .batched import raise_on_err, read_status

COST_NAMES = ["latency_p99", "power", "gpu_over"]
MAX_STEPS_PER_CYCLE = 64      # pacer and update-rate controller, each
MAX_STEPS_UNDER_WINDOW = 1024  # overlapped steps while one advance runs


def expand_mask(bytes_tensor, width):
    """uint8/int bitmask tensor [B] -> bool [B, width]."""
    b = bytes_tensor.to(torch.int64).unsqueeze(1)
    return (b >> torch.arange(width, device=b.device).unsqueeze(0)) & 1 > 0


def pace_train(backlog, n_new, replay_size, interval, world, gate):
    """Turn the transition backlog into train steps: one step per
    ``interval * world`` transitions once ``replay_size`` reaches ``gate``, at
    most MAX_STEPS_PER_CYCLE per call; the rest is carried.  Returns
    ``(steps, backlog)``."""
    backlog += n_new
    steps = 0
    if replay_size >= gate:
        per_step = interval * world
        steps = min(MAX_STEPS_PER_CYCLE, backlog // per_step)
        backlog -= steps * per_step
    return steps, backlog


def make_learner(obs_dim, n_dc, n_g, device, *, world, seed, buffer,
                 sla_p99_ms, power_cap=0.0, energy_budget_j=None, agent=None):
    """The CHSAC-AF agent (unless one is injected) and its replay ring, both
    on ``device``."""
    if agent is None:
        constraints = {"latency_p99": float(sla_p99_ms)}
        if power_cap and power_cap > 0:
            constraints["power"] = float(power_cap)
        if energy_budget_j and energy_budget_j > 0:
            constraints["energy_total"] = float(energy_budget_j)
        constraints["gpu_over"] = 0.0
        agent = make_agent(CHSACAgentConfig(
            obs_dim=obs_dim, n_dc=n_dc, n_g_choices=n_g,
            constraints=constraints, device=str(device),
            graph_capturable=(world == 1)))
    replay = ReplayRing(capacity=int(buffer), obs_dim=obs_dim, n_costs=3,
                        cost_names=COST_NAMES, n_dc=n_dc, n_g=n_g,
                        device=str(device), seed=seed)
    return agent, replay


class ServingWeights:
    """The served actor's seven Linear layers laid out in one flat float
    buffer: per layer the weight transposed to [in][out], then the bias."""

    def __init__(self, agent, buf, obs_dim, n_dc, n_g, hid):
        if not self.servable(agent, obs_dim, n_dc, n_g, hid):
            raise ValueError("agent's actor does not fit the serving layout")
        # (buffer-slice view, source parameter) pairs, so each refresh is a
        # handful of small device-to-device copies
        self.pairs = []
        off = 0
        for lin in self.linears(agent):
            w = lin.weight          # [out, in] -> stored transposed [in][out]
            n = w.numel()
            self.pairs.append((buf[off:off + n].view(w.shape[1], w.shape[0]), w))
            off += n
            b = lin.bias
            self.pairs.append((buf[off:off + b.numel()], b))
            off += b.numel()
        assert off == buf.numel(), (off, buf.numel())

    @staticmethod
    def linears(agent):
        """The 7 Linear layers of the served actor, in buffer-layout order."""
        enc = agent.encoder.net
        return [enc[0], enc[2], enc[4],
                agent.actor.head_dc[0], agent.actor.head_dc[2],
                agent.actor.head_g[0], agent.actor.head_g[2]]

    @classmethod
    def servable(cls, agent, obs_dim, n_dc, n_g, hid) -> bool:
        try:
            shapes = [tuple(l.weight.shape) for l in cls.linears(agent)]
        except (AttributeError, IndexError, TypeError):
            return False
        H = hid
        want = [(H, obs_dim), (H, H), (H, H),
                (H, H), (n_dc, H), (H, H), (n_g, H)]
        return shapes == want and n_dc <= 8 and n_g <= 8 and obs_dim <= 64

    @torch.no_grad()
    def refresh(self):
        """Push the current actor weights into the buffer (after every train
        round; bounds policy staleness together with the kernel's tr_limit
        launch yield)."""
        for dst, src in self.pairs:
            dst.copy_(src.t() if dst.dim() == 2 else src)


def serving_mode(agent, obs_dim, n_dc, n_g, hid, rl_serve, deterministic):
    """``(serve_device, mfma_serve)``: "device" = the actor MLP + masked
    Gumbel-max sampling run INSIDE the advance kernel from the flat weights
    buffer (replicas never pause for a host policy round-trip); "host" =
    pause/resume with a batched forward, on the matrix cores
    (``rl_forward_mfma``, same buffer) unless parity mode or a non-standard
    injected agent forbids it."""
    servable = ServingWeights.servable(agent, obs_dim, n_dc, n_g, hid)
    serve_device = rl_serve == "device"
    if serve_device and not servable:
        warnings.warn("injected agent has non-standard actor dims; "
                      "falling back to host policy serving")
        serve_device = False
    return serve_device, servable and not serve_device and not deterministic


class RLDriver:
    def __init__(self, t, sim, mod, device, *, agent, replay, obs_dim, n_dc,
                 n_g, hid, serve_device, mfma_serve, deterministic=False,
                 use_graph=False, batch=256, warmup=1000, train_interval=256,
                 stats_interval=100, target_updates_per_s=180.0,
                 reserve_cus=16, world=1, logger=None,
                 end_time, events_per_launch, drain_job_rows):
        self.t, self.sim, self.mod, self.device = t, sim, mod, device
        self.rl, self.replay = agent, replay
        self.n_dc, self.n_g, self.hid = n_dc, n_g, hid
        self.serve_device, self.mfma_serve = serve_device, mfma_serve
        self.deterministic = deterministic
        self.use_graph = use_graph
        self.graphed = None  # GraphedSACStep, captured at the first train step
        self.rl_updates = 0
        self.batch, self.warmup = int(batch), int(warmup)
        self.train_interval = int(train_interval)
        self.stats_interval = int(stats_interval)
        # overlapped-loop update-rate target: after each advance window the
        # cycle trains serially until the measured SAC update rate meets
        # this (<=0 disables the controller: throughput mode, training is
        # purely opportunistic).  The standalone hipGraph rate is ~227/s;
        # 180 keeps >1M events/s alongside (measured curve in
        # profiles/README.md: 199 -> 0.74M, 188 -> 0.91M, 149 -> 2.1M,
        # throughput mode -> 5.4M ev/s).
        self.target_ups = float(target_updates_per_s)
        self.reserve_cus = int(reserve_cus)
        self.world = int(world)
        self.logger = logger
        self.end_time, self.events_per_launch = end_time, events_per_launch
        self.drain_job_rows = drain_job_rows
        self.weights = None
        if serve_device or mfma_serve:
            self.weights = ServingWeights(agent, t["policy_weights"], obs_dim,
                                          n_dc, n_g, hid)
            self.weights.refresh()

    # ---------------- per-run() state ----------------
    def start_run(self, timing):
        """Reset the per-run() state and return this run's cycle callable."""
        self.tm = timing
        self.backlog = 0     # transitions not yet converted into train steps
        self._ups_t0 = None  # update-rate controller epoch (first trainable)
        self.dp = self.world > 1 and is_distributed()
        if self.dp or not self.serve_device:
            return self.cycle_sync
        # The advance kernel's blocks are persistent for a whole cycle, so
        # an unmasked launch occupies every wave slot and concurrent train
        # kernels starve (measured: 38 updates/s).  Reserve a small CU
        # island via a CU-masked stream: the advance never dispatches
        # there, and the train stream's kernels land immediately.
        try:
            self.sim.enable_masked_stream(self.reserve_cus)
        except RuntimeError as e:
            # masked stream unavailable: overlap still works, slower
            warnings.warn(f"CU-masked stream unavailable ({e}); "
                          "train kernels may contend with the advance "
                          "kernel")
        # train on a torch-created (NON-BLOCKING) stream: the masked
        # stream is a blocking stream, and the legacy NULL stream
        # implicitly synchronizes with all blocking streams — training
        # on the default stream would serialize behind every advance
        # launch (measured: exactly floor+1 steps/cycle at every island
        # size).  Two non-NULL streams have no implicit ordering.
        self.train_stream = torch.cuda.Stream(device=self.device)
        return self.cycle_overlapped

    def lap(self, key):
        return Lap(self.tm, key)

    # ---------------- the two cycle bodies ----------------
    def cycle_sync(self):
        """One pause/resume cycle: advance, serve the parked requests, ingest,
        train at the transition-paced cadence.  Data-parallel (world > 1 with
        torch.distributed initialized): every rank executes the SAME number of
        cycles and, inside each, the SAME number of SAC train steps — the step
        count comes from globally reduced counters (``dp_sync_step``), so the
        gradient/cost all-reduces inside ``train_step`` are structurally
        paired and no rank can hang waiting for a peer that finished early.
        Returns True when every replica is done."""
        with self.lap("advance_s"):
            self.sim.advance(self.end_time, self.events_per_launch)
            self.tm["launches"] += 1
            st = read_status(self.t, ("err", "done", "n_req", "n_tr", "n_jl"))
        with self.lap("serve_s"):
            if not self.dp:
                # before serving or ingesting anything the overflowed launch
                # produced (dp: every rank raises together after the sync)
                raise_on_err(st["err"])
            self.drain_job_rows(st["n_jl"])
            self.serve(st["n_req"])
            n_new = self.ingest(st["n_tr"])
        # The two warm-up gates differ — a single rank trains once replay
        # holds `warmup` rows, data-parallel ranks only once the smallest
        # replay holds max(warmup, batch).  Both are kept as they were; which
        # one is right is not decided here.
        done, replay_size = st["done"] == 1, self.replay.size
        world, gate = 1, self.warmup
        if self.dp:
            with self.lap("dp_sync_s"):
                err, done, replay_size, n_new = dp_sync_step(
                    st["err"], done, replay_size, n_new)
            raise_on_err(err, some_rank=True)
            world, gate = self.world, max(self.warmup, self.batch)
        steps, self.backlog = pace_train(self.backlog, n_new, replay_size,
                                         self.train_interval, world, gate)
        with self.lap("train_s"):
            self.train(steps)
        return done

    def cycle_overlapped(self):
        """One overlapped cycle: advance on the CU-masked stream, SAC updates
        on the train stream (which owns the reserved CU island) while the
        kernel runs, so training no longer serializes with simulation; then
        sync / ingest / serial train steps up to the target update rate (short
        runs still train even when the whole simulation fits in one cycle) /
        refresh.  Training under the window is opportunistic — with thousands
        of replicas the samples-trained-per-transition ratio stays ~1 like the
        interval-paced cadence, but wall-clock decouples.  Returns True when
        every replica is done."""
        t, tm = self.t, self.tm
        cur = torch.cuda.current_stream(self.device)
        cycle = self.lap("advance_s")
        with self.lap("sync0_s"):
            # the kernel must see last cycle's weight refresh / tr_count reset
            cur.synchronize()
        kernel = self.lap("kernel_s")
        self.sim.advance(self.end_time, self.events_per_launch)
        # train under the advance window (one graph replay at a time, synced
        # so host pacing tracks device completion)
        window = self.lap("train_s")
        gate = max(self.warmup, self.batch)
        can_train = self.replay.size >= gate
        trained = 0
        if can_train:
            ts = self.train_stream
            ts.wait_stream(cur)
            while (trained < MAX_STEPS_UNDER_WINDOW
                   and not self.sim.advance_done()):
                with torch.cuda.stream(ts):
                    self.train(1, refresh=False)
                ts.synchronize()
                trained += 1
        self.sim.advance_sync()
        kernel.stop()
        if can_train:
            # later default-stream ops (floor steps, refresh) must see the
            # side-stream parameter updates
            cur.wait_stream(self.train_stream)
        window.stop()
        with self.lap("status_s"):
            # no n_req: the kernel serves itself, nothing is ever parked
            st = read_status(t, ("err", "done", "n_tr", "n_jl"))
            raise_on_err(st["err"])
        self.drain_job_rows(st["n_jl"])
        with self.lap("ingest_s"):
            self.ingest(st["n_tr"])
        # update-rate controller: train serially until the measured update
        # rate meets the target (the advance kernel's oversubscribed grid
        # head-of-line-blocks concurrent dispatch, so opportunistic overlap
        # alone cannot sustain the standalone train rate — measured)
        with self.lap("floor_s"):
            if self.replay.size >= gate:
                if self._ups_t0 is None:
                    self._ups_t0 = time.perf_counter()
                    self._ups_base = self.rl_updates
                extra = 0
                while self.target_ups > 0 and extra < MAX_STEPS_PER_CYCLE:
                    el = max(1e-6, time.perf_counter() - self._ups_t0)
                    if (self.rl_updates - self._ups_base) >= self.target_ups * el:
                        break
                    self.train(1, refresh=False)
                    extra += 1
                trained += extra
        tm["overlap_train_steps"] += trained
        with self.lap("refresh_s"):
            self.weights.refresh()
        cycle.stop()
        done = st["done"] == 1
        if not done:  # as ever, this loop's count leaves the last launch out
            tm["launches"] += 1
        return done

    # ---------------- serve / ingest / train ----------------
    def serve(self, n_req):
        """Answer the ``n_req`` parked action requests (req_flag == 1) with
        ONE batched policy forward; no other replica is touched."""
        if n_req <= 0:
            return
        t = self.t
        idx = (t["req_flag"] == 1).nonzero(as_tuple=True)[0]
        obs = t["req_obs"][idx]
        m_dc = expand_mask(t["req_mdc"][idx], self.n_dc)
        m_g = expand_mask(t["req_mg"][idx], self.n_g)
        # guard: a fully-false mask wedges the categorical; allow all
        m_dc[m_dc.sum(dim=1) == 0] = True
        m_g[m_g.sum(dim=1) == 0] = True
        if self.deterministic:
            # parity mode: serve one request at a time through the SAME
            # scalar entry the oracle uses, so batch-size-dependent GEMM
            # reduction order can never flip a near-tie argmax
            rows = zip(*(x.cpu().numpy() for x in (obs, m_dc, m_g)))
            acts = [self.rl.select_action(*row, deterministic=True)
                    for row in rows]
            a_dc, a_g = (torch.as_tensor([a[k] for a in acts],
                                         dtype=torch.int32, device=self.device)
                         for k in ("dc", "g"))
        elif self.mfma_serve:
            # matrix-core batched forward (rl_forward_mfma) + the same
            # masked Gumbel-max sampling the torch path uses
            with torch.no_grad():
                ldc, lg = self.mod.rl_forward_mfma(
                    t["policy_weights"], obs.contiguous(),
                    self.hid, self.n_dc, self.n_g)
                a_dc, _ = sample_categorical(ldc, m_dc)
                a_g, _ = sample_categorical(lg, m_g)
        else:
            with torch.no_grad():
                a = self.rl.select_action_batch(obs, m_dc, m_g)
            a_dc, a_g = a["dc"], a["g"]
        t["resp_dc"][idx] = a_dc.to(torch.int32)
        t["resp_g"][idx] = a_g.to(torch.int32)
        t["req_flag"][idx] = 2  # REQ_READY

    def ingest(self, n_tr) -> int:
        """Drain the ``n_tr`` completed transitions from the device ring into
        the replay ring; returns the number ingested."""
        if n_tr <= 0:
            return 0
        t = self.t
        n_tr = min(n_tr, int(t["tr_s0"].shape[0]))
        self.replay.add_batch(
            s=t["tr_s0"][:n_tr], s_next=t["tr_s1"][:n_tr],
            a_dc=t["tr_adc"][:n_tr].to(torch.long),
            a_g=t["tr_ag"][:n_tr].to(torch.long),
            r=t["tr_r"][:n_tr], costs=t["tr_costs"][:n_tr],
            done=torch.ones(n_tr, device=self.device),
            mask_dc=expand_mask(t["tr_mdc"][:n_tr], self.n_dc),
            mask_g=expand_mask(t["tr_mg"][:n_tr], self.n_g))
        t["tr_count"].zero_()
        return n_tr

    def train(self, steps: int, refresh: bool = True):
        """Run `steps` SAC updates: hipGraph-replayed when captured, eager
        otherwise.  Every `stats_interval`-th update runs eagerly with
        compute_stats=True and logs losses/alpha/lambda at INFO — the
        batched-path equivalent of the reference's per-update INFO logging
        (simulator_paper_multi.py:755,807; sampled here because production
        updates are graph-replayed and sync-free).  refresh=False defers the
        serving-buffer update to the caller (the overlapped loop refreshes
        only after the concurrent advance kernel has finished, so the kernel
        never reads a half-copied weight buffer)."""
        if steps <= 0:
            return
        if self.use_graph and self.graphed is None:
            self.graphed = GraphedSACStep(self.rl, self.replay, self.batch)
        for _ in range(steps):
            self.rl_updates += 1
            want_stats = (self.stats_interval > 0 and self.logger is not None
                          and (self.rl_updates == 1 or
                               self.rl_updates % self.stats_interval == 0))
            if want_stats:
                stats = self.rl.train_step(self.replay.sample(self.batch),
                                           compute_stats=True)
                self.logger.info(
                    {"rl_update": self.rl_updates,
                     **{k: round(v, 4) if isinstance(v, (int, float)) else v
                        for k, v in stats.items()}})
            elif self.graphed is not None:
                self.graphed.step()  # one hipGraph replay
            else:
                # sync-free eager SAC step (no stats, tensorized PID)
                self.rl.train_step(self.replay.sample(self.batch),
                                   compute_stats=False)
        if refresh and (self.serve_device or self.mfma_serve):
            self.weights.refresh()
