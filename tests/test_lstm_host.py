"""The host side of the LSTM PPO agents (pednstream_amd/lstm.py) that needs no GPU: the packs' layout, the torch modules beside the
kernels against the reference's recorded outputs (tests/golden/lstm_<case>.npz) and the contract's numpy restatement (tests/lstm_model.py),
and the refusals that are decided before the device is touched."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import lstm_model as lm
from golden_util import GOLDEN
from pednstream_amd import lstm as pl

F = np.float32
AGENTS = [(0, 4, 0, 1), (5, 40, 1, 8), (45, 5, 9, 2)]       # the 50-column table of the SAC tests: an odd slice start, act_w 8
LSTM_FLOATS = lambda ow: 256 * ow + 256 * 64 + 2 * 256


def actors(agents=AGENTS, n_envs=1, n_obs=50, n_actions=11, **kw):
    low, high = np.zeros(n_actions, dtype=F), np.ones(n_actions, dtype=F)
    kw.setdefault("delta_actions", False)
    return pl.LstmActors(agents, low, high, n_envs, n_obs, n_actions, **kw)


def test_tensor_shapes_are_the_references_keys():
    assert pl.actor_tensor_shapes(20, 4) == [("lstm.weight_ih_l0", (256, 20)), ("lstm.weight_hh_l0", (256, 64)), ("lstm.bias_ih_l0", (256,)),
                                             ("lstm.bias_hh_l0", (256,)), ("mean_head.weight", (4, 64)), ("mean_head.bias", (4,)),
                                             ("std_head.weight", (4, 64)), ("std_head.bias", (4,))]
    assert pl.value_tensor_shapes(20)[4:] == [("value_head.weight", (1, 64)), ("value_head.bias", (1,))]
    pytest.importorskip("torch")
    assert [(k, tuple(v.shape)) for k, v in pl.make_actor_module(20, 4).state_dict().items()] == pl.actor_tensor_shapes(20, 4)
    assert [(k, tuple(v.shape)) for k, v in pl.make_value_module(20).state_dict().items()] == pl.value_tensor_shapes(20)
    # the keys and shapes the reference's own classes have
    g = np.load(os.path.join(GOLDEN, "lstm_o20_a4.npz"))
    assert {k[6:]: g[k].shape for k in g.files if k.startswith("actor.")} == dict(pl.actor_tensor_shapes(20, 4))
    assert {k[6:]: g[k].shape for k in g.files if k.startswith("value.")} == dict(pl.value_tensor_shapes(20))


@pytest.mark.parametrize("which", ["actor", "value"])
def test_pack_layout(which):
    shapes = (lambda ow, aw: pl.actor_tensor_shapes(ow, aw)) if which == "actor" else (lambda ow, aw: pl.value_tensor_shapes(ow))
    offsets, total = (pl.actor_pack_layout if which == "actor" else pl.value_pack_layout)(AGENTS)
    assert total % 4 == 0 and len(offsets) == len(AGENTS)
    used = np.zeros(total, dtype=np.int32)
    end = 0
    for (_, ow, _, aw), cur in zip(AGENTS, offsets):
        assert list(cur) == [k for k, _ in shapes(ow, aw)]
        start = cur["lstm.weight_ih_l0"][0]
        assert start % 4 == 0 and 0 <= start - end < 4                   # every agent on the next multiple of 4 floats
        at = start
        for key, shape in shapes(ow, aw):
            assert cur[key] == (at, shape)                               # the tensors lie one behind the other
            used[at:at + int(np.prod(shape))] += 1
            at += int(np.prod(shape))
        end = at
        assert at - start == LSTM_FLOATS(ow) + (2 * (64 * aw + aw) if which == "actor" else 65)
    assert used.max() == 1 and 0 <= total - end < 4
    a = actors()
    t = pl.LstmPpoTargets(a)
    mine = a if which == "actor" else t
    assert mine.pack_size == total and mine.offsets == offsets
    assert a.table.dtype == np.int32 and a.table.shape == (3, 6)
    assert [list(r) for r in a.table] == [[o0, ow, a0, aw, off["lstm.weight_ih_l0"][0], 0] for (o0, ow, a0, aw), off in zip(AGENTS, pl.actor_pack_layout(AGENTS)[0])]
    assert list(t.value_table) == [cur["lstm.weight_ih_l0"][0] for cur in pl.value_pack_layout(AGENTS)[0]]


def test_the_padding_of_a_pack_stays_zero():
    """A pack is a zeroed tensor and a load writes only the tensors' own ranges (packs.views): what lies between two agents is not
    covered by any view."""
    offsets, total = pl.actor_pack_layout(AGENTS)
    covered = np.zeros(total, dtype=bool)
    for cur in offsets:
        for at, shape in cur.values():
            covered[at:at + int(np.prod(shape))] = True
    gaps = np.flatnonzero(~covered)
    assert 0 < len(gaps) < 4 * len(AGENTS) and all(g % 4 != 0 for g in gaps)     # (10 floats of heads per action: agent 0 ends off a multiple of 4)
    torch = pytest.importorskip("torch")
    from pednstream_amd import packs

    pack = torch.zeros(total)
    for (_, ow, _, aw), cur in zip(AGENTS, offsets):
        packs.load(cur, {k: np.full(shape, 7.0, dtype=F) for k, shape in pl.actor_tensor_shapes(ow, aw)}, lambda: pack)
    assert np.array_equal(pack.numpy() == 0, ~covered)


@pytest.mark.parametrize("name", ["o4_a1", "o20_a4", "o6_a2"])
def test_state_dict_round_trip_and_module_forward(name):
    """The reference's state dicts load into the modules beside the kernels; their forward is the reference's (its recorded float32
    outputs, torch's own LSTM both times) and as close to the contract's model as two float32 evaluations of one function are."""
    torch = pytest.importorskip("torch")
    g = np.load(os.path.join(GOLDEN, f"lstm_{name}.npz"))
    info = json.loads(str(g["info_json"]))
    T = info["T"]
    sd = lambda tag: {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + ".")}
    actor, value = pl.make_actor_module(info["obs_dim"], info["act_dim"]), pl.make_value_module(info["obs_dim"])
    actor.load_state_dict({k: torch.as_tensor(v) for k, v in sd("actor").items()})
    value.load_state_dict({k: torch.as_tensor(v) for k, v in sd("value").items()})
    for k, v in actor.state_dict().items():
        assert np.array_equal(v.numpy(), g["actor." + k])
    x = torch.as_tensor(g["obs"])
    with torch.no_grad():
        mu, std, _ = actor(x[None, :T])
        v_all, _ = value.forward_all_steps(x[None, :T])
        v_last, _ = value(x[None, :T])
        nv, _ = value.forward_all_steps(x[None, 1:])
        # stepwise, carrying the hidden state, as take_action does
        hidden, steps = None, []
        for t in range(T):
            m, _, hidden = actor(x[t:t + 1], hidden)
            steps.append(m[0].numpy())
    close = lambda got, k: np.max(np.abs(got.astype(np.float64) - g[k + "64"])) <= 4 * np.max(np.abs(g[k + "32"].astype(np.float64) - g[k + "64"]))
    assert close(mu[0].numpy(), "mu") and close(std[0].numpy(), "std")
    assert close(v_all[0, :, 0].numpy(), "values") and close(nv[0, :, 0].numpy(), "next_values")
    assert v_last.shape == (1, 1) and v_last[0, 0] == v_all[0, -1, 0]
    assert close(np.stack(steps), "mu")
    # and the contract's model on the same state dict
    hs = lm.run(sd("actor"), g["obs"][:T, None, :])[:, 0]
    want_mu, _, want_std = lm.actor_heads(sd("actor"), hs)
    assert close(want_mu, "mu") and close(want_std, "std")


def test_refusals_without_a_device():
    torch = pytest.importorskip("torch")
    from pednstream_amd.rl_env import MultiScenarioVecEnv, VecPedNetEnv

    for kw, msg in (({"hidden_size": 32}, "hidden_size 64"), ({"num_layers": 2}, "num_layers 1"), ({"n_envs": 0}, "must be positive"),
                    ({"agents": []}, "non-empty list"), ({"agents": [(0, 4, 0, 0)]}, "1 to 8 actions"), ({"agents": [(0, 4, 0, 9)]}, "1 to 8 actions"),
                    ({"agents": [(48, 4, 0, 1)]}, "not inside a row"), ({"agents": [(0, 4, 10, 2)]}, "not inside a row"),
                    ({"agents": [(0, 4, 0, 2), (4, 4, 1, 2)]}, "same action column"), ({"agents": [(0, 5, 0, 2)], "delta_actions": True}, "no multiple"),
                    ({"min_std": 0.0}, "min_std"), ({"max_delta": 0.0}, "max_delta"), ({"seed": -1}, "seed"),
                    ({"agent_ids": ["a", "a", "b"]}, "every agent once")):
        with pytest.raises(ValueError, match=msg):
            actors(**kw)
    for make, msg in ((lambda: pl.make_actor_module(4, 1, hidden_size=128), "hidden_size 64"), (lambda: pl.make_value_module(4, num_layers=2), "num_layers 1")):
        with pytest.raises(ValueError, match=msg):
            make()
    with pytest.raises(ValueError, match="LstmActors"):
        pl.LstmPpoTargets(None)
    for name in ("lstm_actors", "lstm_ppo_targets"):
        assert hasattr(VecPedNetEnv, name) and hasattr(MultiScenarioVecEnv, name)
        with pytest.raises(ValueError, match="separate engines"):
            getattr(MultiScenarioVecEnv, name)(None, None)
    with pytest.raises(ValueError, match="one VecPedNetEnv"):
        pl.for_env(object())
    with pytest.raises(ValueError, match="one VecPedNetEnv"):
        pl.targets_for_env(object(), None)
    a = actors(agent_ids=["a", "b", "c"], n_envs=2)
    t = pl.LstmPpoTargets(a)
    for obj in (a, t):
        with pytest.raises(ValueError, match="Unknown agent"):
            obj.load_state_dict("d", {})
        with pytest.raises(ValueError, match="Unknown agent"):
            obj.bind(0, torch.nn.Linear(2, 2))
        with pytest.raises(ValueError, match="do not match"):
            obj.bind("a", torch.nn.Linear(2, 2))                         # foreign parameters, refused before the pack is touched
        with pytest.raises(ValueError, match="do not match"):
            obj.load_state_dict("a", {"lstm.weight_ih_l0": np.zeros((256, 4), F)})
    wrong = {k: np.zeros(s, F) for k, s in pl.actor_tensor_shapes(5, 1)}        # agent "a" has obs_w 4
    with pytest.raises(ValueError, match="expected shape"):
        a.load_state_dict("a", wrong)
    # launches: the tensor checks come first, then the unloaded agents; nothing reaches the device
    for bad, msg in ((None, "must be a torch tensor"), (np.zeros((2, 50), F), "must be a torch tensor"), (torch.zeros(2, 50), "obs must be on cuda:0")):
        with pytest.raises(ValueError, match=msg):
            a.act(bad)
    with pytest.raises(ValueError, match="mask must be"):
        a.reset_hidden(mask=np.zeros(2, bool))
    obs, act = torch.zeros(3, 2, 50), torch.zeros(2, 2, 11)
    for bad in (None, obs.numpy(), torch.zeros(3, 50), torch.zeros(1, 2, 50), torch.zeros(3, 0, 50)):
        with pytest.raises(ValueError, match="obs must be a torch tensor of shape"):
            t.evaluate(bad, act)
    with pytest.raises(ValueError, match="obs must be on cuda:0"):
        t.evaluate(obs, act)
    for call in (lambda: t.evaluate_store(None), lambda: t.compute_gae(None, None, None, 0.99, 0.95)):
        with pytest.raises(ValueError, match="store must be a RolloutStore"):
            call()


def test_gae_refuses_mismatched_next_values_without_a_device():
    torch = pytest.importorskip("torch")
    from pednstream_amd.rollout import gae

    with pytest.raises(ValueError, match="float32 CUDA tensors"):
        gae(torch.zeros(3, 2), torch.zeros(3, 2), torch.zeros(3, 2), 0.99, 0.95, next_values=torch.zeros(3, 2))


def test_the_c_entries_refuse_bad_arguments():
    from pednstream_amd import engine

    lib = engine.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    good = dict(obs=p, table=p, low=p, high=p, params=p, noise=None, hc=p, mu=p, std=p, eps=p, raw=p, actions=p, state=p, n_envs=1, n_obs=1,
                n_actions=1, n_agents=1, hidden=64, layers=1, delta=0, mode=2, max_delta=2.5, min_std=1e-3, max_std=10.0, seed=0, off=0, stream=None)
    bad = [{k: None} for k in ("obs", "table", "low", "high", "params", "hc", "mu", "std", "eps", "raw", "actions", "state")]
    bad += [{"hidden": 32}, {"layers": 2}, {"layers": 0}, {"n_envs": 0}, {"n_obs": 0}, {"n_actions": 0}, {"n_agents": 0}, {"n_agents": 65536},
            {"mode": 3}, {"mode": -1}, {"mode": 1}]                        # (mode 1 without the noise)
    for change in bad:                                                   # every one is refused before anything is launched
        assert lib.pedn_lstm_actor_forward(*{**good, **change}.values()) == -1, change
        assert lib.pedn_last_error(None)
    good = dict(hc=p, mask=None, n_envs=1, n_agents=1, hidden=64, stream=None)
    odd = C.c_void_p(C.addressof(buf) + 4)
    for change in ({"hc": None}, {"hc": odd}, {"n_envs": 0}, {"n_agents": 0}, {"n_agents": 65536}, {"hidden": 32}):
        assert lib.pedn_lstm_reset(*{**good, **change}.values()) == -1, change
    good = dict(obs=p, actions=p, table=p, vtable=p, actor=p, value=p, values=p, next_values=p, logp=p, mu=None, std=None, T=1, N=1, n_obs=1,
                n_actions=1, n_agents=1, hidden=64, layers=1, f64=0, min_std=1e-3, max_std=10.0, stream=None)
    bad = [{k: None} for k in ("obs", "actions", "table", "vtable", "actor", "value", "values", "next_values", "logp")]
    bad += [{"hidden": 32}, {"layers": 2}, {"T": 0}, {"N": 0}, {"n_obs": 0}, {"n_actions": 0}, {"n_agents": 0}, {"n_agents": 65536}, {"f64": 2}, {"f64": -1}]
    for change in bad:
        assert lib.pedn_lstm_ppo_evaluate(*{**good, **change}.values()) == -1, change
    good = dict(rewards=p, values=p, next_values=p, dones=p, T=1, lanes=1, gamma=0.99, lmbda=0.95, td=p, adv=p, stream=None)
    for change in [{k: None} for k in ("rewards", "values", "next_values", "dones", "td", "adv")] + [{"T": 0}, {"lanes": 0}]:
        assert lib.pedn_gae_next(*{**good, **change}.values()) == -1, change
        assert lib.pedn_last_error(None)
