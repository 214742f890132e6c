"""fused_actor_heads off or unusable means unchanged: on the CPU the flag warns
once, falls back, and one update is bit-identical to a default agent's."""
import warnings

import pytest

torch = pytest.importorskip("torch")

from test_critic_mlp_cpu import one_update  # noqa: E402


def test_fused_actor_heads_on_cpu_warns_once_and_changes_nothing():
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        stats, params = one_update(fused_actor_heads=True)
    assert sum("fused_actor_heads" in str(w.message) for w in seen) == 1
    ref_stats, ref_params = one_update()
    assert stats == ref_stats and len(stats) == 4 and len(params) > 30
    assert all(torch.equal(x, y) for x, y in zip(params, ref_params))
