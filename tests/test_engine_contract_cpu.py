"""The replica engine's host <-> device contract, without a GPU.

BatchedSimHip's constructor makes no HIP call: it checks the scalar config
against the kernel's compile-time limits (engine_limits.hpp) and binds every
tensor with dtype, extent, contiguity and device checked (engine_bind.hpp).
So the state of engine/state.py is allocated on the CPU and bound here; the
engine refuses to launch on it.

The limits function is also compiled, with engine_desc.hpp, into a stand-alone
host program under -fsanitize=address,undefined that walks the boundary
values (as test_launch_plan_cpu.py does for the planner).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = os.path.join(REPO, "distributed_cluster_gpus_amd", "ops")
HDR_DIR = os.path.join(OPS, "csrc", "hip")

needs_ext = pytest.mark.skipif(
    not os.path.exists(os.path.join(OPS, "_sim_hip.so")),
    reason="_sim_hip.so not built")

ALGOS = ("default_policy", "cap_uniform", "cap_greedy", "joint_nf", "bandit",
         "carbon_cost", "eco_route", "debug", "chsac_af")
R, TCAP, QCAP, TR_CAP, TRACE_CAP = 3, 8, 16, 32, 4
# tensor dtype -> the name contract() reports for it
DTYPE_NAMES = {torch.float64: "Double", torch.float32: "Float",
               torch.int64: "Long", torch.int32: "Int", torch.int16: "Short",
               torch.int8: "Char", torch.uint8: "Byte"}


@pytest.fixture(scope="module")
def mod():
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    return load_sim_hip("_sim_hip")


def _trace(sc):
    ns = sc.n_ing * 2
    tt = np.cumsum(np.full((R, ns, TRACE_CAP), 0.5), axis=2)
    return tt, np.ones_like(tt)


def _build(sc, algo, *, trace=False, pop_series=False, tcap=TCAP, **rl):
    """(tensors on the CPU, cfg, dims) of one configuration."""
    from distributed_cluster_gpus_amd.configs.paper import build_arrivals
    from distributed_cluster_gpus_amd.engine.state import (alloc_state,
                                                           engine_cfg,
                                                           engine_dims)
    inf, trn = build_arrivals()
    tr = _trace(sc) if trace else None
    dims = engine_dims(sc, algo=algo, n_rep=R, tcap=tcap, qcap=QCAP,
                       tr_cap=TR_CAP, log_replica=0, arrival_trace=tr,
                       pop_series_every=2 if pop_series else 0, **rl)
    return (alloc_state(dims, sc, "cpu", tr),
            engine_cfg(dims, sc, inf, trn), dims)


def _not_dereferenced(dims):
    """Tensors the state holds that this configuration's kernel never reads:
    the placeholders, and the actor-weights buffer unless the kernel serves."""
    out = set()
    if dims.algo != "cap_greedy":
        out.add("snap_f")
    if dims.algo != "bandit":
        out |= {"b_n", "b_s"}
    if dims.is_rl and not dims.exact_p99:
        out |= {"p99_sorted", "p99_ring"}
    return out


def _check_positive(mod, t, cfg, dims):
    sim = mod.BatchedSimHip(t, cfg)
    rows = sim.contract()
    names = [n for n, _, _ in rows]
    assert len(names) == len(set(names))
    required = {n: (dt, need) for n, dt, need in rows if need >= 0}
    unused = {n for n, _, need in rows if need < 0}
    skip = _not_dereferenced(dims)
    assert unused == skip
    # every tensor of the state is bound, except those placeholders and a
    # weights buffer only the host path reads
    want = set(t) - skip
    if not dims.serve_device:
        want.discard("policy_weights")
    assert set(required) == want
    for n, (dt, need) in required.items():
        # equal, not merely sufficient: slack would hide the next drift
        assert t[n].numel() == need, (n, tuple(t[n].shape), need)
        assert dt == DTYPE_NAMES[t[n].dtype], (n, dt, t[n].dtype)
    for call in (lambda: sim.advance(1.0, 10), sim.resident_capacity,
                 lambda: sim.enable_masked_stream(4)):
        with pytest.raises(RuntimeError, match="not on a GPU"):
            call()


@needs_ext
@pytest.mark.parametrize("pop_series", [False, True])
@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
def test_every_algo_binds_exactly_its_state(mod, paper_sc, algo, trace,
                                            pop_series):
    _check_positive(mod, *_build(paper_sc, algo, trace=trace,
                                 pop_series=pop_series))


@needs_ext
@pytest.mark.parametrize("serve", ["host", "device"])
@pytest.mark.parametrize("exact_p99", [False, True])
@pytest.mark.parametrize("elastic", [False, True])
def test_chsac_variants_bind_exactly_their_state(mod, paper_sc, elastic,
                                                 exact_p99, serve):
    t, cfg, dims = _build(paper_sc, "chsac_af", elastic_scaling=elastic,
                          rl_exact_p99=exact_p99,
                          serve_device=serve == "device",
                          weights_buffer=serve == "host")
    assert cfg["elastic"] == int(elastic) and \
        cfg["exact_p99"] == int(exact_p99) and \
        cfg["serve_device"] == int(serve == "device")
    _check_positive(mod, t, cfg, dims)


@needs_ext
def test_eight_lane_build_binds_the_same_contract(paper_sc, mod):
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    t, cfg, dims = _build(paper_sc, "chsac_af", serve_device=True)
    mw = load_sim_hip("_sim_hip_mw").BatchedSimHip(t, cfg)
    assert mw.contract() == mod.BatchedSimHip(t, cfg).contract()


# ---- one rejection per check ------------------------------------------
# two fields of each dtype family (int16 has a single field, s_gpus); the
# chsac state with in-kernel serving holds all of them
FIELDS = ("now", "q_pay",            # float64
          "q_netlat", "req_obs",     # float32
          "busy", "slot_dc",         # int32
          "rng_ctr", "ev_count",     # int64 <-> uint64_t / long long
          "s_gpus",                  # int16 <-> short
          "s_jtype", "q_ing",        # int8 <-> char
          "pp_ing", "tr_adc",        # uint8
          "s_rec", "x_rec")          # float64 rows <-> SRec / XRec


@pytest.fixture(scope="module")
def chsac(paper_sc):
    return _build(paper_sc, "chsac_af", serve_device=True)


def _dropped(x):
    return None


def _one_short(x):
    return x.reshape(-1)[:-1].clone()


def _wrong_dtype(x):
    return x.to(torch.float32 if x.dtype != torch.float32 else torch.float64)


def _non_contiguous(x):
    wide = torch.zeros(*x.shape[:-1], x.shape[-1] * 2, dtype=x.dtype)
    y = wide[..., ::2]
    assert y.shape == x.shape and not y.is_contiguous()
    return y


@needs_ext
@pytest.mark.parametrize("fault", [_dropped, _one_short, _wrong_dtype,
                                   _non_contiguous])
@pytest.mark.parametrize("field", FIELDS)
def test_a_faulty_tensor_is_rejected_by_name(mod, chsac, field, fault):
    t, cfg, _ = chsac
    bad = dict(t)
    y = fault(t[field])
    if y is None:
        del bad[field]
    else:
        bad[field] = y
    with pytest.raises(ValueError, match=f"'{field}': required .* found "):
        mod.BatchedSimHip(bad, cfg)


@needs_ext
@pytest.mark.parametrize("field,width", [("s_rec", 8), ("x_rec", 4)])
def test_record_rows_must_be_as_wide_as_the_record(mod, chsac, field, width):
    t, cfg, _ = chsac
    x = t[field]
    bad = dict(t)
    # one column short, with rows to spare: enough bytes, wrong row width
    bad[field] = torch.zeros(x.shape[0], x.shape[1] * 2, width - 1,
                             dtype=torch.float64)
    assert bad[field].numel() >= x.numel()
    with pytest.raises(ValueError, match=f"'{field}': required .*rows of "
                                         f"{width}.* found .*{width - 1}]"):
        mod.BatchedSimHip(bad, cfg)


@needs_ext
def test_tensors_on_another_device_are_rejected(mod, chsac):
    t, cfg, _ = chsac
    bad = dict(t)
    bad["busy"] = t["busy"].to("meta")
    with pytest.raises(ValueError, match="'busy': required .* on cpu, found "
                                         ".* on meta"):
        mod.BatchedSimHip(bad, cfg)


# ---- limits -----------------------------------------------------------
@needs_ext
@pytest.mark.parametrize("ext", ["_sim_hip", "_sim_hip_mw"])
@pytest.mark.parametrize("key,value,named", [
    ("n_dc", 9, "n_dc = 9"), ("n_ing", 9, "n_ing = 9"),
    ("n_freq", 9, "n_freq = 9"), ("max_gpj", 9, "max_gpj = 9"),
    ("log_replica", R, f"log_replica = {R}"), ("n_dc", 0, "n_dc = 0"),
    ("max_gpj", 0, "max_gpj = 0"), ("algo", 9, "algo = 9"),
    ("log_replica", -2, "log_replica = -2"), ("qcap", 0, "qcap = 0")])
def test_a_dim_past_the_kernels_limits_is_rejected(paper_sc, ext, key, value,
                                                   named):
    from distributed_cluster_gpus_amd.ops import load_sim_hip
    t, cfg, _ = _build(paper_sc, "default_policy")
    with pytest.raises(ValueError, match=named):
        load_sim_hip(ext).BatchedSimHip(t, dict(cfg, **{key: value}))


@needs_ext
def test_the_lds_budget_is_checked_at_construction(mod, paper_sc):
    """64-lane build: the 2 replicas of a block mirror s_finish and x_time in
    LDS, 8 B per slot each; 1488 slots + 2700 transfers alone pass 64 KiB."""
    t, cfg, dims = _build(paper_sc, "default_policy", tcap=2700)
    assert 2 * 8 * (dims.total_slots + 2700) > 64 * 1024
    with pytest.raises(RuntimeError,
                       match=f"total_slots = {dims.total_slots} .* tcap = "
                             "2700 .*64 KiB"):
        mod.BatchedSimHip(t, cfg)
    t, cfg, dims = _build(paper_sc, "default_policy", tcap=1500)
    mod.BatchedSimHip(t, cfg)


@needs_ext
def test_serving_limits_are_checked_at_construction(mod, chsac):
    t, cfg, _ = chsac
    with pytest.raises(ValueError, match="hid = 257"):
        mod.BatchedSimHip(t, dict(cfg, rl_hid=257))
    with pytest.raises(ValueError, match="obs_dim = 65"):
        mod.BatchedSimHip(t, dict(cfg, obs_dim=65))


# ---- the limits function alone, host-only and sanitized ----------------
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <stdexcept>
#include "engine_limits.hpp"

static dcg::EngineDesc good() {
  dcg::EngineDesc S{};
  S.n_rep = 3; S.n_dc = 8; S.n_ing = 8; S.n_streams = 16; S.n_freq = 8;
  S.total_slots = 1488; S.tcap = 8; S.qcap = 16; S.max_gpj = 8;
  S.log_replica = 0; S.cl_cap = 1; S.jl_cap = 1; S.algo = dcg::A_CHSAC;
  S.obs_dim = 49; S.elastic = 1; S.pp_cap = 1; S.p99_win = 1;
  S.serve_device = 1; S.hid = 256; S.n_g = 8;
  return S;
}

static void probe(const char* field, long long v, dcg::EngineDesc S) {
  try {
    dcg::check_engine_limits(S);
    std::printf("%s %lld ok\n", field, v);
  } catch (const std::invalid_argument& e) {
    std::printf("%s %lld %s\n", field, v, e.what());
  }
}

#define WALK(field, ...)                                  \
  for (long long v : {__VA_ARGS__}) {                     \
    dcg::EngineDesc S = good();                           \
    S.field = (int)v;                                     \
    if (!std::strcmp(#field, "n_ing")) S.n_streams = 2 * (int)v; \
    probe(#field, v, S);                                  \
  }

int main() {
  static_assert(sizeof(dcg::SRec) == 64 && sizeof(dcg::XRec) == 32, "");
  probe("good", 0, good());
  WALK(n_dc, 0, 1, 8, 9)
  WALK(n_ing, 0, 1, 8, 9)
  WALK(n_freq, 0, 1, 8, 9)
  WALK(max_gpj, 0, 1, 8, 9)
  WALK(tcap, 0, 1)
  WALK(qcap, 0, 1)
  WALK(total_slots, 0, 1)
  WALK(n_rep, 0, 1)
  WALK(log_replica, -2, -1, 2, 3)
  WALK(cl_cap, 0, 1)
  WALK(jl_cap, 0, 1)
  WALK(algo, -1, 0, 8, 9)
  WALK(obs_dim, 0, 1, 64, 65)
  WALK(pp_cap, 0, 1)
  WALK(p99_win, 0, 1)
  WALK(hid, 0, 1, 256, 257)
  WALK(n_g, 0, 1, 8, 9)
  {  // the chsac and serving checks apply under their switches only
    dcg::EngineDesc S = good();
    S.algo = dcg::A_DEFAULT; S.serve_device = 0;
    S.obs_dim = 0; S.pp_cap = 0; S.p99_win = 0; S.hid = 0; S.n_g = 0;
    probe("ungated", 0, S);
    S = good(); S.elastic = 0; S.pp_cap = 0;
    probe("inelastic", 0, S);
    S = good(); S.n_streams = 15;
    probe("n_streams", 15, S);
  }
  return 0;
}
"""

# field -> the values the walk must accept; everything else it walks is
# rejected with "<field> = <value>" in the message
ACCEPTED = {
    "n_dc": {1, 8}, "n_ing": {1, 8}, "n_freq": {1, 8}, "max_gpj": {1, 8},
    "tcap": {1}, "qcap": {1}, "total_slots": {1}, "n_rep": {1},
    "log_replica": {-1, 2}, "cl_cap": {1}, "jl_cap": {1}, "algo": {0, 8},
    "obs_dim": {1, 64}, "pp_cap": {1}, "p99_win": {1}, "hid": {1, 256},
    "n_g": {1, 8}, "good": {0}, "ungated": {0}, "inelastic": {0},
}


def test_limits_function_host_only_sanitized(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "limits_driver.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "limits_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", HDR_DIR, str(src),
                    "-o", exe], check=True)
    r = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert r.stderr == "", r.stderr   # a sanitizer report
    seen = set()
    for line in r.stdout.splitlines():
        field, v, verdict = line.split(" ", 2)
        v = int(v)
        seen.add(field)
        if v in ACCEPTED.get(field, ()):
            assert verdict == "ok", line
        else:
            named = "n_ing" if field == "n_streams" else field
            assert verdict.startswith("engine limits: ") and \
                f"{named} = " in verdict, line
            if field != "n_streams":
                assert f"{field} = {v}," in verdict, line
    assert seen == set(ACCEPTED) | {"n_streams"}
