"""The host side of PPO's rollout evaluation (pednstream_amd/ppo.py) that needs no GPU: the value pack's layout, the torch module beside
the kernel against the contract's numpy restatement (tests/ppo_eval_model.py), and the refusals that are decided before the device is
touched."""
import ctypes as C

import numpy as np
import pytest

import ppo_eval_model as pm
from pednstream_amd import ppo as pp
from pednstream_amd.policy import StackedActors

F = np.float32
AGENTS = [(0, 4, 0, 1), (5, 40, 1, 8), (45, 5, 9, 2)]       # the 50-column table of the SAC tests: an odd slice start, act_w 8


def test_value_tensor_shapes_are_the_references_keys():
    got = pp.value_tensor_shapes(20, 5)
    assert got == [("encoder.fc1.weight", (64, 100)), ("encoder.fc1.bias", (64,)), ("encoder.fc2.weight", (64, 64)), ("encoder.fc2.bias", (64,)),
                   ("fc.weight", (64, 64)), ("fc.bias", (64,)), ("value_head.weight", (1, 64)), ("value_head.bias", (1,))]
    torch = pytest.importorskip("torch")
    m = pp.make_value_module(20, 5)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == got


@pytest.mark.parametrize("S", [1, 4, 5])
def test_value_pack_layout(S):
    offsets, total = pp.value_pack_layout(AGENTS, S)
    assert total % 4 == 0 and len(offsets) == len(AGENTS)
    used = np.zeros(total, dtype=np.int32)
    end = 0
    for (_, ow, _, _), cur in zip(AGENTS, offsets):
        assert list(cur) == [k for k, _ in pp.value_tensor_shapes(ow, S)]
        start = cur["encoder.fc1.weight"][0]
        assert start % 4 == 0 and 0 <= start - end < 4                   # every agent on the next multiple of 4 floats
        at = start
        for key, shape in pp.value_tensor_shapes(ow, S):
            assert cur[key] == (at, shape)                               # the tensors lie one behind the other
            used[at:at + int(np.prod(shape))] += 1
            at += int(np.prod(shape))
        end = at
        assert at - start == 64 * S * ow + 64 + 2 * (64 * 64 + 64) + 64 + 1 == 64 * S * ow + 8449
    assert used.max() == 1 and 0 <= total - end < 4
    assert (used == 0).sum() == total - sum(64 * S * ow + 8449 for (_, ow, _, _) in AGENTS) == 3 * len(AGENTS)       # 8449 = 1 mod 4
    low, high = np.zeros(11, dtype=F), np.ones(11, dtype=F)
    t = pp.PpoTargets(StackedActors("ppo", AGENTS, low, high, 1, 50, 11, stack_size=S, delta_actions=False))
    assert t.pack_size == total and t.value_table.dtype == np.int32
    assert list(t.value_table) == [cur["encoder.fc1.weight"][0] for cur in offsets]


@pytest.mark.parametrize("obs_w,S", [(4, 4), (20, 5), (6, 1)])
def test_value_module_forward_is_the_models(obs_w, S):
    torch = pytest.importorskip("torch")
    torch.manual_seed(obs_w)
    m = pp.make_value_module(obs_w, S)
    sd = {k: v.numpy() for k, v in m.state_dict().items()}
    x = (np.random.default_rng(S).standard_normal((33, S, obs_w)) * 2).astype(F)
    with torch.no_grad():
        got = m(torch.as_tensor(x))
        got64 = m.double()(torch.as_tensor(x).double())
    want = pm.value(sd, x)
    assert tuple(got.shape) == (33, 1) and want.shape == (33,)
    # the module sums in torch's order, the model in the contract's: both are float32 evaluations of one function
    own = np.abs(got.numpy()[:, 0] - got64.numpy()[:, 0]).max()
    assert np.abs(want - got64.numpy()[:, 0]).max() <= 4 * max(own, 2.0 ** -24 * np.abs(got64.numpy()).max())


def test_refusals_without_a_device():
    torch = pytest.importorskip("torch")
    from pednstream_amd.rl_env import MultiScenarioVecEnv, VecPedNetEnv

    low, high = np.zeros(11, dtype=F), np.ones(11, dtype=F)
    with pytest.raises(ValueError, match="StackedActors"):
        pp.PpoTargets(None)
    with pytest.raises(ValueError, match="kind 'ppo'"):
        pp.PpoTargets(StackedActors("sac", AGENTS, low, high, 1, 50, 11, stack_size=4, delta_actions=False))
    assert hasattr(VecPedNetEnv, "ppo_targets") and hasattr(MultiScenarioVecEnv, "ppo_targets")
    with pytest.raises(ValueError, match="separate engines"):
        MultiScenarioVecEnv.ppo_targets(None, None)
    with pytest.raises(ValueError, match="one VecPedNetEnv"):
        pp.for_env(object(), None)
    t = pp.PpoTargets(StackedActors("ppo", AGENTS, low, high, 1, 50, 11, stack_size=4, delta_actions=False, agent_ids=["a", "b", "c"]))
    with pytest.raises(ValueError, match="Unknown agent"):
        t.load_state_dict("d", {})
    with pytest.raises(ValueError, match="Unknown agent"):
        t.bind(0, torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="do not match"):
        t.bind("a", torch.nn.Linear(2, 2))                               # foreign parameters, refused before the pack is touched
    with pytest.raises(ValueError, match="do not match"):
        t.load_state_dict("a", {"encoder.fc1.weight": np.zeros((64, 16), F)})
    obs, act = torch.zeros(3, 2, 50), torch.zeros(2, 2, 11)
    for bad in (None, obs.numpy(), torch.zeros(3, 50), torch.zeros(1, 2, 50), torch.zeros(3, 0, 50)):
        with pytest.raises(ValueError, match="obs must be a torch tensor of shape"):
            t.evaluate(bad, act)
    with pytest.raises(ValueError, match="obs must be on cuda:0"):
        t.evaluate(obs, act)
    with pytest.raises(ValueError, match="store must be a RolloutStore"):
        t.evaluate_store(None)


def test_the_c_entry_refuses_bad_arguments():
    from pednstream_amd import engine

    lib = engine.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    good = dict(obs=p, actions=p, table=p, vtable=p, actor=p, value=p, values=p, logp=p, mu=None, std=None, T=1, N=1, S=1, n_obs=1, n_actions=1,
                n_agents=1, hidden=64, f64=0, min_std=1e-3, max_std=10.0, stream=None)
    bad = [{k: None} for k in ("obs", "actions", "table", "vtable", "actor", "value", "values", "logp")]
    bad += [{"hidden": 32}, {"T": 0}, {"N": 0}, {"S": 0}, {"n_agents": 0}, {"n_agents": 65536}, {"f64": 2}, {"f64": -1}]
    for change in bad:                                                   # every one is refused before anything is launched
        assert lib.pedn_ppo_evaluate(*{**good, **change}.values()) == -1, change
        assert lib.pedn_last_error(None)
