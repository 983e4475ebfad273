"""Host side of the SAC critic step (pednstream_amd/sac.py: critic_update, critic_gradients): the workspace's shape, the layout of the
gradient pack and its views, and every refusal that needs no GPU."""
import numpy as np
import pytest

from pednstream_amd import engine, packs, sac
from pednstream_amd.policy import StackedActors

AGENTS = [(0, 4, 0, 1), (5, 56, 1, 8), (61, 6, 9, 2)]       # (obs0, obs_w, act0, act_w); the second one starts on an odd column
S = 5


def make():
    actors = StackedActors("sac", AGENTS, low=np.zeros(11), high=np.full(11, 4.0), n_envs=1, n_obs=67, n_actions=11, stack_size=S)
    return sac.SacTargets(actors)


def test_the_entry_point_is_declared():
    import os

    assert "pedn_sac_critic_update" in engine.EXPORTS and engine.ABI_VERSION == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int pedn_sac_critic_update(const float* states" in open(os.path.join(root, "include", "pedn.h")).read()


def test_workspace_shape_and_gradient_views():
    t = make()
    assert sac.CRITIC_TILE == 32
    stride = t.pack_size + 8                                    # 3 agents x 2 losses = 6 floats, rounded up to 4
    assert [t.critic_workspace_shape(B) for B in (1, 32, 33, 130, 1024)] == [(1, stride), (1, stride), (2, stride), (5, stride), (32, stride)]
    assert stride % 4 == 0
    with pytest.raises(ValueError, match="batch size"):
        t.critic_workspace_shape(0)
    # the gradient pack has the layout of the online pack: the same views, in nn.Linear shapes, tiling the pack up to the padding
    torch = pytest.importorskip("torch")
    grads = torch.arange(t.pack_size, dtype=torch.float32)
    covered = np.zeros(t.pack_size, dtype=bool)
    for i, (o0, ow, a0, aw) in enumerate(AGENTS):
        for c in range(2):
            views = packs.views(grads, t.offsets[i][c])
            assert list(views) == [k for k, _ in sac.critic_shapes(ow, aw, S)]
            assert {k: tuple(v.shape) for k, v in views.items()} == dict(sac.critic_shapes(ow, aw, S))
            assert views["fc.weight"].shape == (64, 64 + aw + 1) and views["fc_out.bias"].shape == (1,)
            at = int(t.critic_table[i, c])
            assert at % 4 == 0 and views["encoder.fc1.weight"][0, 0].item() == at
            for k, v in views.items():
                first = int(v.reshape(-1)[0].item())
                assert first == t.offsets[i][c][k][0] and not covered[first:first + v.numel()].any()
                covered[first:first + v.numel()] = True
    assert 0 < (~covered).sum() < 4 * 2 * len(AGENTS)            # only the padding in front of a critic is left


def test_refusals_that_need_no_device():
    torch = pytest.importorskip("torch")
    t = make()
    B = 3
    s, a, td = torch.zeros(B, S, 67), torch.zeros(B, 11), torch.zeros(B, 3)
    for bad in (float("nan"), float("inf"), -1e-3, "x", None):
        with pytest.raises(ValueError, match="lr"):
            t.critic_update(s, a, td, lr=bad)
    for bad in (float("nan"), float("inf"), -1e-8):
        with pytest.raises(ValueError, match="eps"):
            t.critic_update(s, a, td, eps=bad)
    for bad in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, float("nan")), (0.9,), (0.9, 0.99, 0.999), 0.9):
        with pytest.raises(ValueError, match="betas"):
            t.critic_update(s, a, td, betas=bad)
    for bad in (None, np.zeros((B, 3), dtype=np.float32), torch.zeros(B), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match="td_target must"):
            t.critic_update(s, a, bad)
    with pytest.raises(ValueError, match="td_target must be on cuda"):
        t.critic_update(s, a, td)                               # a CPU tensor
    with pytest.raises(ValueError, match="td_target must be on cuda"):
        t.critic_gradients(s, a, td)
    with pytest.raises(ValueError, match="critic_update\\(\\) has not run"):
        t.critic_outputs
    with pytest.raises(ValueError, match="which must be"):
        t.adam_state(0, "critic_3")
    with pytest.raises(ValueError, match="only the online critics"):
        t.adam_state(0, "target_critic_1")
    with pytest.raises(ValueError, match="Unknown agent"):
        t.adam_state(7, "critic_1")
    assert t._cdev is None and t._dev is None                   # nothing above touched a device
