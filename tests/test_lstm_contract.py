"""The contract of the LSTM PPO agents (tests/lstm_model.py) against what the reference's own classes computed
(tests/golden/lstm_<case>.npz, tools/gen_lstm_goldens.py): every output of the model is as close to the reference's float64 evaluation as
4 times the reference's own float32 evaluation is (the margin of sections 14-16).  No GPU."""
import json
import os

import numpy as np
import pytest

import actor_model as am
import lstm_model as lm
import rollout_model as rm
from golden_util import GOLDEN

F = np.float32
CASES = ("o4_a1", "o20_a4", "o56_a8", "o6_a2")
MARGIN = 4.0
_cache = {}


def case(name):
    """The golden and the model's outputs for it: computed once, shared, never written."""
    if name not in _cache:
        g = dict(np.load(os.path.join(GOLDEN, f"lstm_{name}.npz")))
        info = json.loads(str(g["info_json"]))
        agents = [(0, info["obs_dim"], 0, info["act_dim"])]
        sd = lambda tag: {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}
        T = info["T"]
        m = lm.evaluate(agents, [sd("actor")], [sd("value")], g["obs"][:, None, :], g["actions"][:, None, :])
        out = {k: m[k][:, 0] for k in ("mu", "std", "old_log_probs")}
        out["values"], out["next_values"] = m["values"][:, 0, 0], m["next_values"][:, 0, 0]
        open_dones = g["dones"].copy()
        open_dones[-1] = 0
        for tag, d in (("", g["dones"]), ("_open", open_dones)):
            out["td_target" + tag], out["advantage" + tag] = lm.gae_next(g["rewards"], out["values"], out["next_values"], d, float(g["gamma"]), float(g["lmbda"]))
        assert out["values"].shape == (T,)
        _cache[name] = (g, info, out)
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_model_is_as_close_to_float64_as_the_reference_float32(name):
    g, info, out = case(name)
    for k in ("values", "next_values", "mu", "std", "old_log_probs", "td_target", "advantage", "td_target_open", "advantage_open"):
        ref32, ref64 = g[k + "32"], g[k + "64"]
        assert out[k].dtype == F and out[k].shape == ref64.shape, k
        own = np.max(np.abs(ref32.astype(np.float64) - ref64))
        err = np.max(np.abs(out[k].astype(np.float64) - ref64))
        print(f"{name} {k}: model {err:.3e}  reference float32 {own:.3e}  ratio {err / own:.2f}")
        assert own > 0 and err <= MARGIN * own, (name, k, err, own)


@pytest.mark.parametrize("name", CASES)
def test_stepwise_deterministic_actions(name):
    """take_action(deterministic=True) step by step from a fresh hidden state is clamp(mu): the model's stepwise run is its sequence run
    (one function), so its error against the float64 mu is the bound above; the reference's stepwise float32 error is measured."""
    g, info, out = case(name)
    md = float(g["max_delta"])
    ref64 = np.clip(g["mu64"], -md, md)
    own32 = np.max(np.abs(g["mu32"].astype(np.float64) - g["mu64"]))
    step32 = np.max(np.abs(g["det_actions"].astype(np.float64) - ref64))
    mine = am.clip(out["mu"], F(-md), F(md))
    assert np.max(np.abs(mine.astype(np.float64) - g["det_actions"])) <= MARGIN * own32 + step32


def test_next_values_are_a_run_of_their_own():
    """forward_all_steps(next_states) starts from hidden = None at obs[1]: it is not values[1:] (section 16's identity does not carry over)."""
    for name in CASES:
        g, _, out = case(name)
        for v, nv in ((g["values32"], g["next_values32"]), (g["values64"], g["next_values64"]), (out["values"], out["next_values"])):
            assert not np.array_equal(nv[:-1], v[1:])
            assert np.max(np.abs(nv[:-1] - v[1:])) > 1e-4


def test_sigmoid_and_tanh_against_double():
    """The contract's float64 forms over float32 arguments from 1e-6 to 30, both signs: within 2^-40 relative of numpy's double."""
    z = np.concatenate([np.geomspace(1e-6, 30.0, 150000), 2.0 ** -13 * (1 + np.linspace(-1e-3, 1e-3, 2001))]).astype(F)
    z = np.concatenate([z, -z])
    zd = z.astype(np.float64)
    t, want = lm.tanh64(z), np.tanh(zd)
    assert np.max(np.abs(t - want) / np.abs(want)) <= 2.0 ** -40
    assert np.array_equal(np.signbit(t), np.signbit(zd))
    s, want = lm.sigmoid64(z), 1.0 / (1.0 + np.exp(-zd))
    assert np.max(np.abs(s - want) / want) <= 2.0 ** -40
    # the ends: zeros keep their sign, saturation is exact, NaN stays
    edge = np.array([0.0, -0.0, 600.0, -600.0, np.inf, -np.inf, 3e38, -3e38, np.nan], dtype=F)
    t, s = lm.tanh(edge), lm.sigmoid(edge)
    assert np.array_equal(t[:8], np.array([0.0, -0.0, 1, -1, 1, -1, 1, -1], dtype=F)) and np.signbit(t[1]) and not np.signbit(t[0]) and np.isnan(t[8])
    assert np.array_equal(s[:8], np.array([0.5, 0.5, 1, 0, 1, 0, 1, 0], dtype=F)) and np.isnan(s[8])


def test_gae_with_next_values_is_the_rollout_contract():
    """next_values := values[1:] gives rollout_model.td_and_gae bit for bit."""
    rng = np.random.default_rng(5)
    for T, shape in ((1, (1,)), (7, (3, 2)), (37, (5,))):
        r = rng.standard_normal((T,) + shape).astype(F)
        v = rng.standard_normal((T + 1,) + shape).astype(F)
        d = (rng.random((T,) + shape) < 0.2).astype(F)
        td, adv = lm.gae_next(r, v[:-1], v[1:], d, 0.99, 0.95)
        td0, adv0 = rm.td_and_gae(r, v, d, 0.99, 0.95)
        assert np.array_equal(td, td0) and np.array_equal(adv, adv0)
