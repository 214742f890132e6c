#!/usr/bin/env python3
"""Geo GPU cluster simulator CLI (MI355X-native framework).

Flag surface and output-directory rule are compatible with the reference CLI
(reference: run_sim_paper.py:11-160); outputs are the same cluster_log.csv /
job_log.csv / project.log triple.

Extensions over the reference:
  --engine {oracle,native,batched}   pick the scalar Python oracle, the C++
                                     DES core, or the batched MI355X engine
  --replicas N                       Monte-Carlo replicas (batched engine)
  --pop-series [EVERY]               per-tick mean/CI bands over the replica
                                     ensemble (batched engine)
  --latency-hist                     latency tail quantiles and SLA misses
                                     over the replica ensemble (batched engine)
  --inf-mode profile / --trn-mode profile
                                     per-ingress piecewise-constant arrival
                                     rates (--inf-profile / --trn-profile FILE,
                                     or --ingress-tz-offsets-h for a sinusoid
                                     shifted per ingress), every engine
  --sweep-inf-rate / --sweep-trn-rate / --sweep-power-cap A,B,..
                                     a grid of parameter points inside one
                                     replica ensemble (batched engine)
  --eco-objective is actually honored (the reference parses but drops it,
    SURVEY Appendix A.4), and --elastic-scaling is a store_true flag that
    really enables elastic scaling (the reference's type=bool flag could
    never be True).
"""
import argparse
import os


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description="Geo GPU Simulator (MI355X-native, multi-ingress)",
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)

    # --- core ---
    p.add_argument("--duration", type=float, default=180.0,
                   help="Total simulated time (seconds).")
    p.add_argument("--policy", type=str, default="energy_aware",
                   choices=["energy_aware", "perf_first"],
                   help="In-DC heuristic allocation policy.")
    p.add_argument("--log-interval", type=float, default=5.0,
                   help="Cluster/job log cadence (seconds).")
    p.add_argument("--log-path", type=str, default=None, help="Log path")
    p.add_argument("--seed", type=int, default=123, help="Random seed.")
    p.add_argument("--progress", default=True,
                   help="Show a tqdm progress bar over simulated time.")

    # --- arrivals (inference) ---
    p.add_argument("--inf-mode", type=str, default="sinusoid",
                   choices=["poisson", "sinusoid", "off", "profile"])
    p.add_argument("--inf-rate", type=float, default=6.0)
    p.add_argument("--inf-amp", type=float, default=0.6)
    p.add_argument("--inf-period", type=float, default=300.0)

    # --- arrivals (training) ---
    p.add_argument("--trn-mode", type=str, default="poisson",
                   choices=["poisson", "sinusoid", "off", "profile"])
    p.add_argument("--trn-rate", type=float, default=0.3)
    p.add_argument("--trn-period", type=float, default=3600.0,
                   help="Cycle of a training rate profile (seconds).")

    # --- per-ingress rate profiles (mode 'profile') ---
    for kind in ("inf", "trn"):
        p.add_argument(f"--{kind}-profile", type=str, default=None,
                       metavar="FILE",
                       help=f"--{kind}-mode profile: CSV of n_ing rows (or one "
                            "shared row) x K <= 64 columns of rate "
                            f"multipliers; --{kind}-rate scales them and "
                            f"--{kind}-period is the cycle.")
    p.add_argument("--ingress-tz-offsets-h", type=_float_list, default=None,
                   metavar="H0,H1,..",
                   help="--inf-mode profile without --inf-profile: one "
                        "time-zone offset in hours per ingress; the table is "
                        "the --inf-rate/--inf-amp/--inf-period sinusoid in 24 "
                        "segments, shifted per ingress by H/24 of the period "
                        "(the period stands for one day).")

    # --- algorithm / controller ---
    p.add_argument("--algo", type=str, default="default_policy",
                   choices=["default_policy", "cap_uniform", "cap_greedy",
                            "joint_nf", "bandit", "carbon_cost",
                            "eco_route", "chsac_af", "debug"])
    p.add_argument("--elastic-scaling", action="store_true", default=False,
                   help="Enable elastic scaling (RL algo only).")
    p.add_argument("--power-cap", type=float, default=0.0,
                   help="Total power cap (W); only cap_uniform/cap_greedy, <=0 = off.")
    p.add_argument("--control-interval", type=float, default=5.0,
                   help="Controller cadence (seconds).")
    p.add_argument("--use-control-interval", action="store_true", default=False,
                   help="Actually fire the cap controller at --control-interval "
                        "(the reference parses the flag but fires at "
                        "log-interval; default keeps that parity).")
    p.add_argument("--eco-objective", type=str, default="energy",
                   choices=["energy", "carbon", "cost"])
    # debug params
    p.add_argument("--num_fixed_gpus", type=int, default=1)
    p.add_argument("--fixed_freq", type=float, default=None)

    # --- RL knobs ---
    p.add_argument("--upgr-buffer", type=int, default=200_000)
    p.add_argument("--upgr-batch", type=int, default=256)
    p.add_argument("--upgr-warmup", type=int, default=1_000)
    p.add_argument("--upgr-device", type=str, default="cuda", choices=["cuda", "cpu"])
    p.add_argument("--sla_p99_ms", type=float, default=500.0)
    p.add_argument("--energy_budget_j", type=float, default=None)

    # --- MI355X-framework extensions ---
    p.add_argument("--engine", type=str, default="oracle",
                   choices=["oracle", "native", "batched"],
                   help="oracle = Python DES; native = C++ DES core; "
                        "batched = MI355X HIP replica engine.")
    p.add_argument("--replicas", type=int, default=4096,
                   help="Monte-Carlo replicas (batched engine only).")
    p.add_argument("--pop-series", type=int, nargs="?", const=1, default=0,
                   metavar="EVERY",
                   help="Batched engine only: sample every replica at every "
                        "EVERY-th log tick and write the per-tick population "
                        "statistics to <out>/population/population_series.csv "
                        "(0 = off).")
    p.add_argument("--latency-hist", action="store_true", default=False,
                   help="Batched engine only: every replica histograms its "
                        "job latencies per DC and job type; writes tail "
                        "quantiles and SLA-miss fractions with confidence "
                        "bands over the replicas to <out>/population/"
                        "latency_quantiles.csv and the pooled histogram to "
                        "latency_hist.csv (SLA: --sla_p99_ms).")
    for flag, what in (("--sweep-inf-rate", "inference arrival rates"),
                       ("--sweep-trn-rate", "training arrival rates"),
                       ("--sweep-power-cap", "power caps in W (cap_greedy)")):
        p.add_argument(flag, type=_float_list, default=None, metavar="A,B,..",
                       help=f"Batched engine only: comma list of {what}; the "
                            "--sweep-* lists together form a grid of "
                            "parameter points, --replicas are split evenly "
                            "over them, and per-point statistics go to "
                            "<out>/population/sweep.csv.")
    p.add_argument("--rl-serve", type=str, default="device",
                   choices=["device", "host"],
                   help="chsac_af policy serving on the batched engine: "
                        "in-kernel actor (device) or host pause/resume.")
    p.add_argument("--rl-exact-p99", action="store_true", default=False,
                   help="Exact 2048-sample sliding-window p99 on the batched "
                        "engine (parity mode) instead of the histogram "
                        "approximation.")
    p.add_argument("--rl-target-ups", type=float, default=180.0,
                   help="chsac_af batched engine: SAC update-rate target for "
                        "the overlapped loop (<=0 = pure-throughput mode).")
    p.add_argument("--fp32-coeff-eval", action="store_true", default=False,
                   help="fp32 decision-score evaluation in the sim kernels "
                        "(batched engine; times/energies stay f64).")
    p.add_argument("--single-dc", action="store_true", default=False,
                   help="Use the single-DC debug topology.")
    p.add_argument("--rl-checkpoint", type=str, default=None,
                   help="Path to save the RL agent checkpoint at the end "
                        "(chsac_af only).")
    p.add_argument("--rl-resume", type=str, default=None,
                   help="Path to an RL agent checkpoint to load before running.")
    args = p.parse_args(argv)
    if sweep_axes(args) and args.engine != "batched":
        p.error("--sweep-inf-rate / --sweep-trn-rate / --sweep-power-cap "
                "need --engine batched")
    return args


def _float_list(text):
    try:
        vals = [float(x) for x in text.split(",") if x.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a comma list of numbers: {text!r}")
    if not vals:
        raise argparse.ArgumentTypeError("an empty list")
    return vals


def sweep_axes(args):
    """The --sweep-* lists as Sweep.grid axes, in flag order ({} = no sweep)."""
    given = (("inf_rate", args.sweep_inf_rate), ("trn_rate", args.sweep_trn_rate),
             ("power_cap", args.sweep_power_cap))
    return {name: vals for name, vals in given if vals is not None}


def profile_arrival(kind, mode, rate, amp, period, path, offsets_h, n_ing):
    """The ArrivalProcess of one job type from the CLI flags: the plain modes
    as before; 'profile' from its CSV file, or (inference) from the per-ingress
    time-zone offsets."""
    from distributed_cluster_gpus_amd.models.arrivals import ArrivalProcess
    if mode != "profile":
        return ArrivalProcess(mode=mode, rate=rate, amp=amp, period=period)
    if kind == "trn" and not path:
        raise SystemExit("--trn-mode profile needs --trn-profile FILE")
    if path:
        ap = ArrivalProcess.from_csv(path, rate=rate, period=period, amp=amp)
    elif kind == "inf" and offsets_h:
        ap = ArrivalProcess.diurnal(
            rate, amp, period, [h / 24.0 * period for h in offsets_h],
            segments=24)
    else:
        raise SystemExit(f"--{kind}-mode profile needs --{kind}-profile FILE"
                         + (" or --ingress-tz-offsets-h" if kind == "inf"
                            else ""))
    ap.profile_rows(n_ing)        # 1 or n_ing rows, or ValueError
    return ap


def resolve_out_dir(log_path, algo):
    """Reference output-dir rule (run_sim_paper.py:136-140): a bare name gets
    the algo appended; a path containing a separator is used as-is."""
    if log_path:
        norm = os.path.normpath(log_path)
        return os.path.join(norm, algo) if os.sep not in norm else norm
    return os.getcwd()


def main(argv=None):
    args = parse_args(argv)

    from distributed_cluster_gpus_amd.configs.paper import (
        build_arrivals, paper_scenario, single_dc_scenario)
    from distributed_cluster_gpus_amd.models.gputypes import validate_gpu_specs
    from distributed_cluster_gpus_amd.models.scenario import PolicyParams
    from distributed_cluster_gpus_amd.utils.logging import get_logger

    policy = PolicyParams(name=args.policy)
    sc = single_dc_scenario(policy=policy) if args.single_dc else paper_scenario(policy=policy)

    warnings = validate_gpu_specs((sc.gpu_specs[n] for n in sc.dc_names), strict=False)
    for m in warnings:
        print("[GPU VALIDATION]", m)

    # (a 'profile' type is built below, from its table)
    plain = {"profile": "off"}
    arrival_inf, arrival_trn = build_arrivals(
        inf_mode=plain.get(args.inf_mode, args.inf_mode),
        inf_rate=args.inf_rate, inf_amp=args.inf_amp,
        inf_period=args.inf_period,
        trn_mode=plain.get(args.trn_mode, args.trn_mode),
        trn_rate=args.trn_rate)
    if "profile" in (args.inf_mode, args.trn_mode):
        arrival_inf = profile_arrival(
            "inf", args.inf_mode, args.inf_rate, args.inf_amp, args.inf_period,
            args.inf_profile, args.ingress_tz_offsets_h, sc.n_ing)
        arrival_trn = profile_arrival(
            "trn", args.trn_mode, args.trn_rate, arrival_trn.amp,
            args.trn_period if args.trn_mode == "profile"
            else arrival_trn.period, args.trn_profile, None, sc.n_ing)
    sc.arrival_inf, sc.arrival_trn = arrival_inf, arrival_trn

    out_dir = resolve_out_dir(args.log_path, args.algo)
    logger = get_logger(out_dir)

    rl_device = args.upgr_device
    if rl_device == "cuda":
        import torch
        if not torch.cuda.is_available():
            rl_device = "cpu"

    common = dict(
        algo=args.algo, duration=args.duration, log_interval=args.log_interval,
        out_dir=out_dir, seed=args.seed, power_cap=args.power_cap,
        control_interval=args.control_interval,
        elastic_scaling=args.elastic_scaling, eco_objective=args.eco_objective,
        use_control_interval=args.use_control_interval,
        num_fixed_gpus=args.num_fixed_gpus, fixed_freq=args.fixed_freq,
        sla_p99_ms=args.sla_p99_ms, energy_budget_j=args.energy_budget_j,
        rl_device=rl_device, rl_batch=args.upgr_batch,
        rl_warmup=args.upgr_warmup, rl_buffer=args.upgr_buffer,
        logger=logger,
        show_progress=(str(args.progress).lower() not in ("false", "0", "no")))

    if args.engine == "native":
        from distributed_cluster_gpus_amd.engine.native import NativeEngine
        eng = NativeEngine(sc, arrival_inf, arrival_trn, **common)
    elif args.engine == "batched":
        from distributed_cluster_gpus_amd.engine.batched import BatchedEngine
        from distributed_cluster_gpus_amd.engine.sweep import Sweep
        axes = sweep_axes(args)
        eng = BatchedEngine(sc, arrival_inf, arrival_trn,
                            sweep=Sweep.grid(**axes) if axes else None,
                            replicas=args.replicas, rl_serve=args.rl_serve,
                            rl_exact_p99=args.rl_exact_p99,
                            rl_target_updates_per_s=args.rl_target_ups,
                            fp32_coeff_eval=args.fp32_coeff_eval,
                            pop_series=args.pop_series > 0,
                            pop_series_every=max(1, args.pop_series),
                            latency_hist=args.latency_hist,
                            **common)
    else:
        from distributed_cluster_gpus_amd.engine.oracle import OracleEngine
        eng = OracleEngine(sc, arrival_inf, arrival_trn, **common)

    if args.rl_resume and getattr(eng, "rl", None) is not None:
        eng.rl.load(args.rl_resume)

    stats = eng.run()
    if args.engine == "batched" and args.replicas > 1:
        # Monte-Carlo population report: distributions over the replica
        # ensemble (a capability the scalar reference cannot express)
        from distributed_cluster_gpus_amd.analysis.montecarlo import \
            population_report
        rep = population_report(eng, out_dir=os.path.join(out_dir, "population"))
        e = rep.get("total_energy_kJ")
        if e:
            print(f"[population] {rep['replicas']} replicas: total energy "
                  f"{e['mean']:.1f} kJ ± {e['stderr']:.2f} (95% CI "
                  f"[{e['ci_lo']:.1f}, {e['ci_hi']:.1f}])")
    if args.engine == "batched" and args.pop_series > 0:
        from distributed_cluster_gpus_amd.analysis.montecarlo import \
            population_series_report
        sdf = population_series_report(
            eng, out_dir=os.path.join(out_dir, "population"))
        print(f"[population] time series: {sdf['time_s'].nunique()} ticks -> "
              f"{os.path.join(out_dir, 'population', 'population_series.csv')}")
    if args.engine == "batched" and args.latency_hist:
        from distributed_cluster_gpus_amd.analysis.montecarlo import \
            latency_report
        latency_report(eng, out_dir=os.path.join(out_dir, "population"),
                       logger=logger)
        print("[population] latency quantiles -> "
              f"{os.path.join(out_dir, 'population', 'latency_quantiles.csv')}")
    if args.engine == "batched" and eng.sweep is not None:
        from distributed_cluster_gpus_amd.analysis.montecarlo import \
            sweep_report
        wdf = sweep_report(eng, out_dir)
        print(f"[population] sweep: {len(wdf)} parameter points -> "
              f"{os.path.join(out_dir, 'population', 'sweep.csv')}")
    if args.rl_checkpoint and getattr(eng, "rl", None) is not None:
        eng.rl.save(args.rl_checkpoint)
        print(f"RL checkpoint saved to {args.rl_checkpoint}")

    print(f"Done. ({args.algo}) Logs: cluster_log.csv, job_log.csv")
    print(f"[perf] events={stats['events']} wall_s={stats['wall_s']:.3f} "
          f"events_per_sec={stats['events_per_sec']:.1f} "
          f"rl_updates={stats.get('rl_updates', 0)} "
          f"jobs_completed={stats.get('jobs_completed', 0)}")
    return stats


if __name__ == "__main__":
    main()
