"""The contract of PPO's rollout evaluation as tests/ppo_eval_model.py restates it, against what the reference's own
PPOAgent computed (tests/golden/ppoeval_*.npz, recorded by tools/gen_ppo_eval_goldens.py): no GPU needed.  The margin is the one of
sections 14 and 15: the model may be off the reference's float64 pipeline by at most 4 times what the reference's own float32 pipeline is
off it."""
import collections
import glob
import json
import os

import numpy as np
import pytest

import ppo_eval_model as pm
import rollout_model as rm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("o4_a1_s4", "o20_a4_s5", "o56_a8_s5", "o6_a2_s1")
F = np.float32
MARGIN = 4.0

_cache = {}


def golden(case):
    """The fixture and the model's outputs for it, computed once per case and never written."""
    if case not in _cache:
        g = dict(np.load(os.path.join(GOLDEN, f"ppoeval_{case}.npz")))
        info = json.loads(str(g["info_json"]))
        sd = lambda tag: {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}
        agents = [(0, info["obs_dim"], 0, info["act_dim"])]
        out = pm.evaluate(agents, [sd("actor")], [sd("value")], g["obs"][:, None, :], g["actions"][:, None, :], info["stack_size"])
        _cache[case] = (g, info, {k: (v[:, 0, 0] if k == "values" else v[:, 0]) for k, v in out.items()})
    return _cache[case]


def test_all_cases_are_there():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "ppoeval_*.npz"))) == sorted(f"ppoeval_{c}.npz" for c in CASES)
    for c in CASES:
        g, info, _ = golden(c)
        T = info["T"]
        assert T == 37 and g["obs"].shape == (T + 1, info["obs_dim"]) and g["actions"].shape == (T, info["act_dim"])
        assert g["dones"][-1] == 1.0 and not g["dones"][:-1].any()
        assert 0.05 <= g["std32"].min() and g["std32"].max() <= 10.0
        assert np.abs(g["actions"]).max() <= g["max_delta"]
        assert (g["obs"] == 0).any() and np.signbit(g["obs"][g["obs"] == 0]).any() and not np.signbit(g["obs"][g["obs"] == 0]).all()


@pytest.mark.parametrize("S", [1, 4, 5])
@pytest.mark.parametrize("T", [1, 2, 7])
def test_stacks_are_the_references_deque(S, T):
    rng = np.random.default_rng(10 * S + T)
    obs = rng.standard_normal((T + 1, 3, 6)).astype(F)
    got = pm.stacks(obs, S)
    assert got.shape == (T + 1, 3, S, 6) and got.dtype == F
    for e in range(3):
        queue = collections.deque(maxlen=S)                    # PPO_org.py:250-257: S copies of the reset observation ...
        for _ in range(S):
            queue.append(obs[0, e])
        assert np.array_equal(got[0, e], np.array(queue))
        for t in range(T):                                     # ... :296-297: one append per step; the next stack of row t is the stack of t + 1
            queue.append(obs[t + 1, e])
            assert np.array_equal(got[t + 1, e], np.array(queue)), (t, e)
    assert np.array_equal(pm.stack_times(T, S)[:, -1], np.arange(T + 1))


@pytest.mark.parametrize("case", CASES)
def test_next_values_are_the_values_one_row_on(case):
    g, _, _ = golden(case)
    for w in ("32", "64"):
        assert np.array_equal(g["next_values" + w][:-1], g["values" + w][1:]), w


def ratio(model, ref32, ref64):
    own = np.max(np.abs(ref32.astype(np.float64) - ref64))
    err = np.max(np.abs(model.astype(np.float64) - ref64))
    return err / own, err, own


@pytest.mark.parametrize("case", CASES)
def test_model_is_within_the_references_own_float32_error(case):
    g, info, out = golden(case)
    ref = {w: {"values": np.append(g["values" + w], g["next_values" + w][-1]), "mu": g["mu" + w], "std": g["std" + w],
               "old_log_probs": g["old_log_probs" + w]} for w in ("32", "64")}
    for k in ("values", "mu", "std", "old_log_probs"):
        assert out[k].dtype == F and out[k].shape == ref["64"][k].shape, k
        r, err, own = ratio(out[k], ref["32"][k], ref["64"][k])
        print(f"{case} {k}: model error {err:.3e}, the reference's float32 error {own:.3e}, ratio {r:.2f}")
        assert err <= MARGIN * own, (case, k, r)


@pytest.mark.parametrize("case", CASES)
def test_td_target_and_advantages_through_the_rollout_model(case):
    g, info, out = golden(case)
    gamma, lmbda = float(g["gamma"]), float(g["lmbda"])
    open_dones = g["dones"].copy()
    open_dones[-1] = 0.0
    for tag, dones in (("", g["dones"]), ("_open", open_dones)):
        td, adv = rm.td_and_gae(g["rewards"], out["values"], dones, gamma, lmbda)
        for k, v in (("td_target", td), ("advantage", adv)):
            r, err, own = ratio(v, g[k + tag + "32"], g[k + tag + "64"])
            print(f"{case} {k}{tag}: model error {err:.3e}, the reference's float32 error {own:.3e}, ratio {r:.2f}")
            assert err <= MARGIN * own, (case, k + tag, r)
    # a done last row cuts the bootstrap value off; an open one lets it in
    assert np.array_equal(g["td_target32"][-1:], g["rewards"][-1:]) and g["td_target_open32"][-1] != g["rewards"][-1]
