"""Host side of the SAC actor and temperature step (pednstream_amd/sac.py: actor_update, actor_gradients): the entry point, the
workspace's shape, the target entropies and every refusal that needs no GPU."""
import numpy as np
import pytest

from pednstream_amd import engine, sac
from pednstream_amd.policy import StackedActors

AGENTS = [(0, 4, 0, 1), (5, 56, 1, 8), (61, 6, 9, 2)]       # (obs0, obs_w, act0, act_w); the second one starts on an odd column
S = 5


def make():
    actors = StackedActors("sac", AGENTS, low=np.zeros(11), high=np.full(11, 4.0), n_envs=1, n_obs=67, n_actions=11, stack_size=S)
    return sac.SacTargets(actors)


def test_the_entry_point_is_declared():
    import os

    assert "pedn_sac_actor_update" in engine.EXPORTS and engine.ABI_VERSION == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int pedn_sac_actor_update(const float* states" in open(os.path.join(root, "include", "pedn.h")).read()
    assert engine.EXPORTS.index("pedn_sac_actor_update") > engine.EXPORTS.index("pedn_sac_critic_update")      # an addition, behind what was there


def test_workspace_shape_and_target_entropies():
    t = make()
    pack = t.actors.pack_size
    assert pack == sum(64 * S * ow + 64 + 2 * (64 * 64 + 64) + 2 * (64 * aw + aw) for (_, ow, _, aw) in AGENTS) + 2      # 2: the padding behind agent 0
    stride = -(-pack // 4) * 4 + 8                              # 3 agents x 2 sums = 6 floats, rounded up to 4
    assert [t.actor_workspace_shape(B) for B in (1, 32, 33, 130, 1024)] == [(1, stride), (1, stride), (2, stride), (5, stride), (32, stride)]
    assert stride % 4 == 0
    with pytest.raises(ValueError, match="batch size"):
        t.actor_workspace_shape(0)
    assert t._target_entropy(None).tolist() == [-1.0, -8.0, -2.0] and t._target_entropy(None).dtype == np.float32      # -act_w
    assert t._target_entropy(-3).tolist() == [-3.0] * 3 and t._target_entropy([0.5, -1, 2]).tolist() == [0.5, -1.0, 2.0]
    assert sac.ACTOR_ACTION_OUTPUTS[:5] == ("mu", "std", "eps", "logp", "new_actions") and sac.ACTOR_AGENT_OUTPUTS == ("entropy", "q1", "q2")


def test_refusals_that_need_no_device():
    torch = pytest.importorskip("torch")
    t = make()
    B = 3
    s, nz = torch.zeros(B, S, 67), torch.zeros(B, 11)
    for bad in (float("nan"), float("inf"), -1e-3, "x", None):
        with pytest.raises(ValueError, match="lr"):
            t.actor_update(s, nz, actor_lr=bad)
        with pytest.raises(ValueError, match="lr"):
            t.actor_update(s, nz, alpha_lr=bad)
    for bad in (float("nan"), float("inf"), -1e-8):
        with pytest.raises(ValueError, match="eps"):
            t.actor_update(s, nz, eps=bad)
    for bad in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, float("nan")), (0.9,), (0.9, 0.99, 0.999), 0.9):
        with pytest.raises(ValueError, match="betas"):
            t.actor_update(s, nz, betas=bad)
    for bad in (float("nan"), float("-inf"), [0.0, float("nan"), 0.0]):
        with pytest.raises(ValueError, match="target_entropy must be finite"):
            t.actor_update(s, nz, target_entropy=bad)
    for bad in ([1.0, 2.0], [[1.0, 2.0, 3.0]], np.zeros(4)):
        with pytest.raises(ValueError, match="target_entropy must be a number or 3 numbers"):
            t.actor_gradients(s, nz, target_entropy=bad)
    with pytest.raises(ValueError, match="target_entropy must be a number"):
        t.actor_update(s, nz, target_entropy="low")
    for bad in (None, np.zeros((B, S, 67), dtype=np.float32), torch.zeros(B, 67), torch.zeros(0, S, 67)):
        with pytest.raises(ValueError, match="states must"):
            t.actor_update(bad, nz)
    with pytest.raises(ValueError, match="states must be on cuda"):
        t.actor_update(s, nz)                                   # a CPU tensor
    with pytest.raises(ValueError, match="states must be on cuda"):
        t.actor_gradients(s)
    with pytest.raises(ValueError, match="actor_update\\(\\) has not run"):
        t.actor_outputs
    with pytest.raises(ValueError, match="Unknown agent"):
        t.actor_adam_state(7)
    assert t._adev is None and t._dev is None and t.actors._dev is None      # nothing above touched a device
