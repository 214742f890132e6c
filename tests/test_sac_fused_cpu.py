"""fused_critic off or unusable means unchanged: on the CPU the flag warns
once, falls back, and trains bit-identically to a default agent."""
import warnings

import pytest

torch = pytest.importorskip("torch")

from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,  # noqa: E402
                                                   CHSACAgentConfig)


def two_updates(fused_critic):
    torch.manual_seed(7)
    agent = CHSACAgent(CHSACAgentConfig(
        obs_dim=13, n_dc=3, n_g_choices=4, constraints={"latency_p99": 500.0},
        device="cpu", fused_critic=fused_critic))
    B = 32
    batch = {"s": torch.randn(B, 13), "s_next": torch.randn(B, 13),
             "a_dc": torch.randint(0, 3, (B,)), "a_g": torch.randint(0, 4, (B,)),
             "r": torch.randn(B), "done": (torch.arange(B) % 2).float(),
             "costs": {"latency_p99": torch.rand(B) * 900},
             "mask_dc": torch.rand(B, 3) < 0.8, "mask_g": torch.rand(B, 4) < 0.8}
    for _ in range(2):
        agent.train_step(batch)
    return agent.state_dict()


def flat(x):
    if isinstance(x, dict):
        return [t for k in sorted(x, key=str) for t in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in flat(v)]
    return [x] if torch.is_tensor(x) else []


def test_fused_critic_on_cpu_warns_once_and_changes_nothing():
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        fused = two_updates(True)
    assert sum("fused_critic" in str(w.message) for w in seen) == 1
    ref = two_updates(False)
    a, b = flat({k: v for k, v in fused.items() if k != "cfg"}), \
        flat({k: v for k, v in ref.items() if k != "cfg"})
    assert len(a) == len(b) > 50
    assert all(torch.equal(x, y) for x, y in zip(a, b))
