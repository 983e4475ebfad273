"""Host side of the stacked actors (pednstream_amd/policy.py): the parameter pack's layout, the agent table and every refusal that needs
no GPU."""
import numpy as np
import pytest

from pednstream_amd import policy
from pednstream_amd.policy import StackedActors, agent_table, pack_layout

AGENTS = [(0, 4, 0, 1), (5, 56, 1, 8), (61, 6, 9, 2)]       # (obs0, obs_w, act0, act_w); the second one starts on an odd column


def make(kind="sac", agents=AGENTS, **kw):
    args = dict(low=np.zeros(11), high=np.full(11, 4.0), n_envs=3, n_obs=67, n_actions=11, stack_size=5)
    args.update(kw)
    return StackedActors(kind, agents, **args)


def numel(kind, obs_w, act_w, S):
    return 64 * S * obs_w + 64 + 2 * (64 * 64 + 64) + (128 if kind == "ppo" else 0) + 2 * (act_w * 64 + act_w)


@pytest.mark.parametrize("kind", ["sac", "ppo"])
def test_pack_offsets_and_table(kind):
    S = 5
    offsets, total = pack_layout(kind, AGENTS, S)
    at = 0
    for (o0, ow, a0, aw), off in zip(AGENTS, offsets):
        at = -(-at // 4) * 4
        assert off["encoder.fc1.weight"] == (at, (64, S * ow))
        keys = list(off)
        assert keys[:6] == ["encoder.fc1.weight", "encoder.fc1.bias", "encoder.fc2.weight", "encoder.fc2.bias", "fc.weight", "fc.bias"]
        assert keys[-4:] == ["fc_mu.weight", "fc_mu.bias", "fc_std.weight", "fc_std.bias"]
        assert (keys[6:-4] == ["ln.weight", "ln.bias"]) == (kind == "ppo") and len(keys) == (12 if kind == "ppo" else 10)
        pos = at
        for k in keys:                                   # one tensor behind the other, no gaps
            assert off[k][0] == pos
            pos += int(np.prod(off[k][1]))
        assert pos - at == numel(kind, ow, aw, S)
        assert off["fc_mu.weight"][1] == (aw, 64) and off["fc_std.bias"][1] == (aw,)
        at = pos
    assert total == at
    table = agent_table(kind, AGENTS, S)
    assert table.dtype == np.int32 and table.shape == (3, policy.TABLE_COLS)
    assert table[:, :4].tolist() == [list(a) for a in AGENTS]
    assert table[:, 4].tolist() == [off["encoder.fc1.weight"][0] for off in offsets] and not table[:, 5].any()
    actors = make(kind)
    assert actors.pack_size == total and np.array_equal(actors.table, table) and actors.agent_ids == [0, 1, 2]


def test_constructor_refusals():
    with pytest.raises(ValueError, match="hidden_size"):
        make(hidden_size=128)
    with pytest.raises(ValueError, match="kind"):
        make(kind="td3")
    with pytest.raises(ValueError, match="stack_size"):
        make(stack_size=0)
    with pytest.raises(ValueError, match="observation columns"):
        make(agents=[(60, 8, 0, 1)])
    with pytest.raises(ValueError, match="action columns"):
        make(agents=[(0, 4, 10, 2)])
    with pytest.raises(ValueError, match="1 to 8 actions"):
        make(agents=[(0, 18, 0, 9)])
    with pytest.raises(ValueError, match="no multiple"):
        make(agents=[(0, 7, 0, 2)])
    make(agents=[(0, 7, 0, 2)], delta_actions=False)
    with pytest.raises(ValueError, match="same action column"):
        make(agents=[(0, 4, 0, 2), (4, 4, 1, 2)])
    with pytest.raises(ValueError, match="low and high"):
        make(low=np.zeros(3))
    with pytest.raises(ValueError, match="agent_ids"):
        make(agent_ids=["a", "a", "b"])


def test_state_dict_refusals():
    actors = make("sac", agent_ids=["g0", "g1", "s0"])
    sd = {k: np.zeros(shape, dtype=np.float32) for k, (_, shape) in actors.offsets[1].items()}
    with pytest.raises(ValueError, match="Unknown agent"):
        actors.load_state_dict("nobody", sd)
    with pytest.raises(ValueError, match="Unknown agent"):
        actors.parameters("nobody")
    with pytest.raises(ValueError, match="ln"):
        actors.load_state_dict("g1", dict(sd, **{"ln.weight": np.ones(64), "ln.bias": np.zeros(64)}))
    with pytest.raises(ValueError, match="shape"):
        actors.load_state_dict("g0", sd)                 # g1's shapes
    with pytest.raises(ValueError, match="keys"):
        actors.load_state_dict("g1", {k: v for k, v in sd.items() if k != "fc.bias"})
    ppo = make("ppo")
    with pytest.raises(ValueError, match="ln"):
        ppo.load_state_dict(1, sd)


def test_act_refusals_without_a_gpu():
    torch = pytest.importorskip("torch")
    actors = make()
    with pytest.raises(ValueError, match="torch tensor"):
        actors.act(np.zeros((3, 5, 67), dtype=np.float32))
    with pytest.raises(ValueError, match="cuda"):
        actors.act(torch.zeros(3, 5, 67))


def test_multi_scenario_env_refuses():
    from pednstream_amd.rl_env import MultiScenarioVecEnv

    env = MultiScenarioVecEnv.__new__(MultiScenarioVecEnv)     # (the refusal needs no engine)
    env.groups = []
    with pytest.raises(ValueError, match="MultiScenarioVecEnv"):
        env.stacked_actors(kind="sac")
    with pytest.raises(ValueError, match="MultiScenarioVecEnv"):
        policy.for_env(env)
