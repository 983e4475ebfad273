"""The preconditions of tests/test_gpu_wide_agents.py, checked on the CPU: the inputs of tests/wide_agents.py reach the paths they are
there for.  Conditions on the reference model alone (tests/rl_oracle.py on the C oracle, the fixtures recorded from the reference) --
nothing here looks at the engine."""
import numpy as np
import pytest

import wide_agents as wa
from pednstream_amd.agents import RuleBasedSeparatorAgent
from pednstream_amd.flatten import flatten_network
from rl_oracle import RlOracle
from test_controllers_host import load
from test_rl_golden import agent_spec


def test_hub8_is_one_gater_with_eight_links():
    adj, params, origins, dests = wa.hub8()
    assert adj.shape == (17, 17) and adj[0].sum() == 8 and 0 not in origins and 0 not in dests
    assert all(adj[o].sum() == 1 for o in origins)                       # the origins are leaves
    assert params["controllers"] == {"enabled": True, "nodes": [0]} and len(params["links"]) == 2
    net = wa.hub8_network()
    assert flatten_network(net)["max_degree"] == 8
    assert agent_spec(net) == wa.HUB_SPEC
    links = [net.links[(0, k)] for k in range(1, 9)]
    assert len({l.width for l in links}) > 1 and len({l.k_critical for l in links}) > 1 and len({l.length for l in links}) > 1
    net.close()


def seq_mean(v):
    return wa.SequentialSum.mean(v)


def test_reward_mean_replicas_tell_numpys_summation_order_from_the_sequential_one():
    """At least 5 (replica, step) pairs of the reward-mean batch in which the float32 reward changes when its two means are summed left
    to right, at least one under each action gap."""
    counts = {}
    for gap in (1, 2):
        acts, obs, rew, seq = wa.reward_models(gap)
        counts[gap] = int((rew.view(np.uint32) != seq.view(np.uint32)).sum())
        dens = obs[:, :, 2::4]
        print(f"action_gap {gap}: {counts[gap]} of {rew.size} (replica, step) rewards differ; densities: mean {dens.mean():.2f}, "
              f"{(dens > 4).mean():.3f} above 4, {(dens == 0).mean():.3f} exactly 0")
        assert (dens > 4).any() and (dens < 4).mean() > 0.8
    assert min(counts.values()) >= 1 and sum(counts.values()) >= 5, counts


def gater_inputs(case):
    """[steps, 8] densities the gater decided on at every step of a hub8 fixture"""
    z, info = load(case)
    obs = z["state_ctrl_obs"]
    seen = np.vstack([z["state_ctrl_reset_obs"][:1], obs[:-1]])
    return seen[:, 2::4], z["state_ctrl_actions"], info


def test_hub8_fixtures_take_every_branch_of_the_gater_rule():
    """avg <= 2 and avg > 2 at least 10 steps each; with threshold 0.0 a link of density exactly 0.0 while avg > 2 (the `==` arm: the
    action is the link's physical width, not current - 1) in at least 3 steps; above and below the threshold 3."""
    for case in ("ctrl_hub8_gate", "ctrl_hub8_gate0"):
        dens, acts, info = gater_inputs(case)
        avg = np.array([np.mean(list(d)) for d in dens])
        thr = np.float32(info["controllers"]["gate_0"]["threshold"])
        rule = dens[avg > 2]
        n_eq, n_above, n_below = (int(m.any(axis=1).sum()) for m in (rule == thr, rule > thr, rule < thr))
        print(f"{case}: avg <= 2 in {(avg <= 2).sum()} steps, > 2 in {(avg > 2).sum()}; under the rule a link equal to / above / below "
              f"the threshold in {n_eq} / {n_above} / {n_below} steps")
        assert (avg <= 2).sum() >= 10 and (avg > 2).sum() >= 10
        assert n_above >= 3
        if case == "ctrl_hub8_gate0":
            assert n_eq >= 3
            widths = np.float32(info["controllers"]["gate_0"]["widths"])
            hit = (avg > 2)[:, None] & (dens == 0)
            assert (acts[hit] == np.broadcast_to(widths, acts.shape)[hit]).all()
        else:
            assert n_below >= 3


def test_summation_order_of_the_gaters_average_is_not_observable_in_these_inputs():
    """The only place where the order of the gater's `avg` sum can show is the comparison with 2.  Over every hub8 input of these tests
    (both fixtures, the reward-mean replicas) the sequential float32 mean differs from np.mean in many steps but never falls on the other
    side of 2: the 8-way order of THAT sum is not pinned through the actions.  (It is the same device function, numpy_sum_f32, whose order
    the rewards pin.)  Should an input ever be found, this test fails and the replica belongs into the GPU test."""
    differ = other_side = 0
    rows = [gater_inputs(c)[0] for c in ("ctrl_hub8_gate", "ctrl_hub8_gate0")] + [wa.reward_models(g)[1][:, :, 2::4].reshape(-1, 8) for g in (1, 2)]
    for dens in rows:
        for d in dens:
            a, b = np.mean(list(d)), seq_mean(d)
            differ += a != b
            other_side += (a <= 2) != (b <= 2)
    print(f"sequential avg differs in {differ} steps, on the other side of 2 in {other_side}")
    assert differ > 50 and other_side == 0


CHECKED = sorted(set(wa.CORRIDOR_CHECKED[70]) | set(wa.CORRIDOR_CHECKED[320]))


def zero_runs(x):
    """lengths of the runs of exact zeros between two nonzero values, and of the run at the end"""
    nz = np.flatnonzero(x != 0)
    inner = [int(b - a - 1) for a, b in zip(nz[:-1], nz[1:]) if b - a > 1]
    return inner, int(len(x) - 1 - nz[-1])


@pytest.mark.parametrize("w", [8, 13, 32])
def test_sparse_corridor_demand_fills_and_empties_every_window(w):
    """For every checked replica the outflow the separator agent of window w is handed holds a run of zeros at least w long behind a full
    window (the action returns to width / 2), a shorter run between two pulses, and a step at which a nonzero value is the oldest of a
    full window whose other values are zero -- evicted one step later, the action flips from about `width` to width / 2: a ring that is
    off by one flips a step early or late."""
    for r in CHECKED:
        x, acts = wa.corridor_series(w, r)
        inner, tail = zero_runs(x)
        assert max(inner + [tail]) >= w and min(inner) < w, (w, r, inner, tail)
        flips = [k for k in range(w - 1, len(x) - 1) if x[k - w + 1] != 0 and not x[k - w + 2:k + 2].any()]
        assert flips, (w, r)
        k = flips[0]
        assert acts[k + 1] > 0.9 * 4 and acts[k + 2] == 2.0, (w, r, k, acts[k:k + 3])


def test_corridor_series_is_the_host_agents_own():
    """corridor_series drives the oracle with pednstream_amd.agents, which the ctrl_corridor_sep_w* fixtures pin at these windows"""
    x, acts = wa.corridor_series(8, 0)
    ag = RuleBasedSeparatorAgent(4, use_smoothing=True, buffer_size=8)
    mine = [ag.take_action(np.float32([0, 0, 0, 0]))[0]] + [ag.take_action(np.float32([0, v, 0, 0]))[0] for v in x[:-1]]
    assert np.array_equal(np.float32(mine), acts[:len(mine)])
