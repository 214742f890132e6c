"""fused_critic_mlp off or unusable means unchanged: on the CPU the flag warns
once, falls back, and one update is bit-identical to a default agent's."""
import warnings

import pytest

torch = pytest.importorskip("torch")

from distributed_cluster_gpus_amd.rl.agent import (CHSACAgent,  # noqa: E402
                                                   CHSACAgentConfig)


def one_update(**flags):
    torch.manual_seed(7)
    agent = CHSACAgent(CHSACAgentConfig(
        obs_dim=13, n_dc=3, n_g_choices=4, constraints={"latency_p99": 500.0},
        device="cpu", **flags))
    B = 32
    batch = {"s": torch.randn(B, 13), "s_next": torch.randn(B, 13),
             "a_dc": torch.randint(0, 3, (B,)), "a_g": torch.randint(0, 4, (B,)),
             "r_eff": torch.randn(B), "done": (torch.arange(B) % 2).float(),
             "mask_dc": torch.rand(B, 3) < 0.8, "mask_g": torch.rand(B, 4) < 0.8}
    stats = agent.algo.update(batch)
    return stats, [p.detach().clone() for p in agent.algo.parameters()] + \
        [agent.algo.log_alpha.detach().clone()]


def test_fused_critic_mlp_on_cpu_warns_once_and_changes_nothing():
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        stats, params = one_update(fused_critic_mlp=True)
    assert sum("fused_critic_mlp" in str(w.message) for w in seen) == 1
    ref_stats, ref_params = one_update()
    assert stats == ref_stats and len(stats) == 4
    assert len(params) == len(ref_params) > 30
    assert all(torch.equal(x, y) for x, y in zip(params, ref_params))
