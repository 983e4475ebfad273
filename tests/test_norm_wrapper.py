"""pednstream_amd.normalize without a GPU: the host RunningMeanStd is the reference's, the wrapper delegates to its env and goes
through VecPedNetEnv's normalisation interface (a stand-in here), statistics round-trip in the reference's dict layout, and
compat.install() exposes both classes as rl.rl_utils."""
import sys

import numpy as np
import pytest

from norm_model import batch_moments, merge
from pednstream_amd.normalize import RunningMeanStd, RunningNormalizeWrapper


def test_running_mean_std_is_the_reference_update():
    rng = np.random.default_rng(0)
    rms = RunningMeanStd(shape=(5,))
    mean, var, count = np.zeros(5), np.ones(5), 1e-4
    for n in (1, 1, 7, 64):
        x = rng.standard_normal((n, 5))
        rms.update(x)
        mean, var, count = merge(mean, var, count, np.mean(x, axis=0), np.var(x, axis=0), n)
        assert np.array_equal(rms.mean, mean) and np.array_equal(rms.var, var) and rms.count == count
    one = RunningMeanStd(shape=(5,))          # one row: np.mean is the row, np.var is 0 -- the contract's N = 1 case
    row = rng.standard_normal((1, 5))
    one.update(row)
    bm, bv = batch_moments(row)
    assert np.array_equal(bm, row[0]) and not bv.any()
    assert np.array_equal(one.mean, merge(np.zeros(5), np.ones(5), 1e-4, bm, bv, 1)[0])


class _Vec:
    possible_agents = ["sep_0_1", "gate_2"]

    def __init__(self):
        self.calls, self.stats = [], None

    def norm_layout(self):
        return np.array([1, 1, 1, 1, 1, 1, 0, 1, 1, 0], dtype=bool), np.array([0] * 4 + [1] * 6, dtype=np.int32)

    def set_running_norm(self, **kw):
        self.calls.append(("set_running_norm", kw))
        self.stats = {"obs_rms": {"sep_0_1": {"mean": [0.0] * 4, "var": [1.0] * 4, "count": 1e-4},
                                  "gate_2": {"mean": [0.0] * 4, "var": [1.0] * 4, "count": 1e-4}}}
        if kw["norm_reward"]:
            self.stats["ret_rms"] = {"mean": 0.0, "var": 1.0, "count": 1e-4}

    def set_training(self, training):
        self.calls.append(("set_training", training))

    def get_normalization_stats(self):
        return self.stats

    def set_normalization_stats(self, stats):
        self.stats = stats

    def true_rewards(self):
        return np.float32([[-3.5, 0.25]])


class _Env:
    possible_agents = _Vec.possible_agents
    marker = "delegated"

    def __init__(self):
        self._vec = _Vec()

    def reset(self, **kw):
        return {"sep_0_1": np.zeros(4, np.float32), "gate_2": np.zeros(6, np.float32)}, {"sep_0_1": {"kw": kw}}

    def step(self, actions):
        return ({}, {"sep_0_1": -1.0, "gate_2": 0.5}, {a: False for a in self.possible_agents}, {a: False for a in self.possible_agents},
                {"sep_0_1": {"step": 2}})


def test_wrapper_delegates_and_round_trips_statistics():
    env = _Env()
    w = RunningNormalizeWrapper(env, norm_obs=True, norm_reward=True, clip_obs=7.0, gamma=0.5, training=False)
    assert env._vec.calls == [("set_running_norm", dict(norm_obs=True, norm_reward=True, clip_obs=7.0, clip_reward=10.0, gamma=0.5, training=False))]
    assert w.marker == "delegated" and w.possible_agents == env.possible_agents and w.env is env
    with pytest.raises(AttributeError):
        w.no_such_attribute
    assert (w.norm_obs, w.norm_reward, w.clip_obs, w.clip_reward, w.gamma, w.training) == (True, True, 7.0, 10.0, 0.5, False)
    obs, infos = w.reset(options={"randomize": False})
    assert infos["sep_0_1"]["kw"] == {"options": {"randomize": False}}
    _, rewards, _, _, infos = w.step({})
    assert rewards == {"sep_0_1": -1.0, "gate_2": 0.5}
    assert infos["sep_0_1"] == {"step": 2, "true_reward": -3.5} and infos["gate_2"] == {"true_reward": 0.25}
    w.set_training(True)
    assert w.training and env._vec.calls[-1] == ("set_training", True)
    saved = {"obs_rms": {"sep_0_1": {"mean": [1.0, 2.0, 3.0, 4.0], "var": [0.5] * 4, "count": 12.0001},
                         "gate_2": {"mean": [0.1] * 4, "var": [2.0] * 4, "count": 12.0001}},
             "ret_rms": {"mean": -2.0, "var": 9.0, "count": 24.0001}}
    w.set_normalization_stats(saved)
    assert w.get_normalization_stats() == saved
    assert w.obs_rms["gate_2"].mean.shape == (4,) and w.obs_rms["sep_0_1"].count == 12.0001 and w.ret_rms.var == 9.0
    with pytest.raises(TypeError):
        RunningNormalizeWrapper(object())


def test_compat_exposes_the_classes_as_rl_rl_utils():
    from pednstream_amd import compat

    before = {k: v for k, v in sys.modules.items() if k in ("src", "handlers", "rl") or k.startswith(("src.", "handlers.", "rl."))}
    try:
        compat.install(force=True)
        from rl.rl_utils import RunningMeanStd as A, RunningNormalizeWrapper as B

        assert A is RunningMeanStd and B is RunningNormalizeWrapper
    finally:
        for k in [k for k in sys.modules if k in ("src", "handlers", "rl") or k.startswith(("src.", "handlers.", "rl."))]:
            del sys.modules[k]
        sys.modules.update(before)
