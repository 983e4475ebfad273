"""The running-normalisation contract (tests/norm_model.py) on the CPU: at one env it IS the reference's
RunningNormalizeWrapper -- bit for bit against what the reference returned for three golden episodes (tests/golden/norm_*.npz,
tools/gen_norm_goldens.py) --, and at N > 1 its fixed-order batch moments stay within the standard summation bound of numpy's."""
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, Golden
from norm_model import NormModel, batch_moments, fixed_sum, merge

CASES = ["nine_opt3", "corridor_opt1", "i45_episode"]
FLAGS = ["obs", "obsrew"]
FPL = {"option1": 3, "option2": 4, "option3": 5, "option4": 2, "option5": 7}


def layout(rl):
    """(tracked mask, agent of column) of a golden's agent list."""
    tracked, agent = [], []
    for i, a in enumerate(rl["agents"]):
        if a["type"] == "sep":
            tracked += [True] * 4
            agent += [i] * 4
        else:
            f = FPL[rl["obs_mode"]]
            tracked += ([True] * (f - 1) + [False]) * len(a["links"])
            agent += [i] * (f * len(a["links"]))
    return np.array(tracked), np.array(agent)


def load_norm(case, flags):
    z = np.load(os.path.join(GOLDEN, f"norm_{case}_{flags}.npz"), allow_pickle=False)
    return z, json.loads(str(z["info_json"]))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("case", CASES)
def test_one_env_is_the_reference_wrapper(case, flags):
    z, info = load_norm(case, flags)
    g = Golden("rl_" + case)
    tracked, agent = layout(g.info["rl"])
    model = NormModel(1, tracked, agent, len(info["agents"]), clip_obs=info["clip_obs"], clip_reward=info["clip_reward"], gamma=info["gamma"],
                      **info["flags"])
    obs, rew, term = g.state("rl_obs"), g.state("rl_rewards"), g.state("rl_terminated")
    assert (~tracked).sum() == sum(len(a["links"]) for a in g.info["rl"]["agents"] if a["type"] == "gate")
    model.reset()
    o = model.observe(z["reset_obs"][None])
    assert np.array_equal(o[0].view(np.uint32), z["reset_obs_n"].view(np.uint32))
    for k in range(info["steps"]):
        if k == info["frozen_from"]:
            model.training = False
        o = model.observe(obs[k:k + 1])
        r = model.rewards(rew[k:k + 1], term[k])
        assert np.array_equal(o[0].view(np.uint32), z["obs_n"][k].view(np.uint32)), k
        assert np.array_equal(r[0].view(np.uint32), z["rew_n"][k].astype(np.float32).view(np.uint32)), k
        assert np.array_equal(o[0][~tracked], obs[k][~tracked])
    assert np.array_equal(z["true_rew"], rew.astype(np.float64))
    s = model.stats(info["agents"])
    assert np.array_equal(np.concatenate([s["obs_rms"][a]["mean"] for a in info["agents"]]), z["mean"])
    assert np.array_equal(np.concatenate([s["obs_rms"][a]["var"] for a in info["agents"]]), z["var"])
    assert np.array_equal(np.array([s["obs_rms"][a]["count"] for a in info["agents"]]), z["count"])
    if info["flags"]["norm_reward"]:
        assert np.array_equal(np.array([s["ret_rms"][k] for k in ("mean", "var", "count")]), z["ret_rms"])
        assert not z["true_rew"].any() or not np.array_equal(z["rew_n"], z["true_rew"])        # (a separator is never rewarded)
    else:
        assert "ret_rms" not in s and np.array_equal(z["rew_n"], z["true_rew"])


def test_the_fixed_order_is_the_documented_tree():
    x = np.random.default_rng(1).standard_normal(200) * 1e3
    strands = [x[s::64] for s in range(64)]
    leaves = []
    for st in strands:
        acc = st[0]
        for v in st[1:]:
            acc = acc + v
        leaves.append(acc)
    while len(leaves) > 1:
        leaves = [leaves[i] + leaves[i + 1] for i in range(0, len(leaves), 2)]
    assert fixed_sum(x) == leaves[0]
    assert fixed_sum(x[:1]) == x[0] and fixed_sum(x[:3]) == (x[0] + x[1]) + x[2]
    assert fixed_sum(x[:65]) == fixed_sum(np.concatenate([[x[0] + x[64]], x[1:64]]))


@pytest.mark.parametrize("n", [2, 3, 64, 65, 200])
def test_batch_moments_within_the_summation_bound_of_numpy(n):
    """Any summation order of N terms is within (N - 1) u sum|x_i| <= N u N max|x| of the exact sum (u = 2^-53), so two orders' MEANS
    differ by at most 2 N u max|x|; the issue's bounds 4 N u max|x| (mean) and 8 N u max|x|^2 (variance) leave the factor two for the
    deviations being taken from slightly different means."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n, 37)) * rng.uniform(0.1, 500.0, size=37) + rng.uniform(-100, 100, size=37)).astype(np.float32)
    x64 = x.astype(np.float64)
    bm, bv = batch_moments(x64)
    big = np.abs(x64).max(axis=0)
    assert (np.abs(bm - np.mean(x64, axis=0)) <= 4 * n * 2.0 ** -53 * big).all()
    assert (np.abs(bv - np.var(x64, axis=0)) <= 8 * n * 2.0 ** -53 * big ** 2).all()
    # ... and so does the merge into running statistics (the same operations on both sides)
    m0, v0, c0 = rng.standard_normal(37), rng.uniform(0.5, 2.0, 37), 10.0
    mine = merge(m0, v0, c0, bm, bv, n)
    theirs = merge(m0, v0, c0, np.mean(x64, axis=0), np.var(x64, axis=0), n)
    assert (np.abs(mine[0] - theirs[0]) <= 4 * n * 2.0 ** -53 * np.maximum(big, np.abs(m0))).all()
    assert (np.abs(mine[1] - theirs[1]) <= 8 * n * 2.0 ** -53 * np.maximum(big, np.abs(m0)) ** 2 + 4 * 2.0 ** -53 * v0).all()
    assert mine[2] == theirs[2] == c0 + n
