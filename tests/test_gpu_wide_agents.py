"""GPU tests of the RL observation / reward kernel and the on-device controllers where no scenario under data/ takes them: a gater with 8
outgoing links (the second pass of rl_observe_body's per-wave link loop, LDS rows 4..7, observation columns 4*fpl..8*fpl, NumPy's 8-way
pairwise summation in the reward's means and in the gater's average), moving-average windows of 1, 8, 13 and 32 values, the `density ==
threshold` arm of the gater rule, and replicas beyond the first group of 64 and in the second half-batch chain.  Inputs and their
preconditions: tests/wide_agents.py, tests/test_wide_agents_host.py.  Every comparison is bitwise.

The fixtures ctrl_hub8_gate, ctrl_hub8_gate0 and ctrl_corridor_sep_w1 / _w8 / _w13 / _w32 run step by step for one env in
test_gpu_controllers.py::test_controlled_steps_reproduce_the_reference_fixture (they are entries of CTRL_CASES)."""
import functools

import numpy as np
import pytest

import sparse_oracle as so
import wide_agents as wa
from golden_util import ALL_FIELDS, Golden, build_network
from pednstream_amd.flatten import flatten_network
from pednstream_amd.network import LINK_FIELDS
from pednstream_amd.rl_env import VecPedNetEnv
from rl_oracle import RlOracle
from test_controllers_host import host_agents, load
from test_gpu_controllers import PLANS, device_agents, make_env

pytestmark = pytest.mark.gpu

STEPS = 120


def set_plan(monkeypatch, plan):
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def hub8_oracle(mode, normalize, gap, replicas, B):
    """{replica: (obs [STEPS, O], rewards [STEPS, 1], {field: [links, rows]})} of RlOracle under hub8_actions(gap, B, STEPS)"""
    net = wa.hub8_network()
    model = flatten_network(net)
    acts = wa.hub8_actions(gap, B, STEPS)
    out = {}
    for r in replicas:
        o = RlOracle(net, model, wa.HUB_SPEC, mode, normalize, gap, seed=wa.HUB_SEED, replica=r, reward_mode="all")
        rows = [o.step(acts[k, r]) for k in range(STEPS)]
        assert o.o.flags() == 0
        out[r] = (np.array([x for x, _ in rows]), np.array([w for _, w in rows]), {f: o.o.field(f)[:model["n_links"], :STEPS * gap + 1] for f in ALL_FIELDS})
    net.close()
    return out


def run_hub8(mode, normalize, gap, reward_mode, B, replicas, history="full"):
    want = hub8_oracle(mode, normalize, gap, replicas, B)
    acts = wa.hub8_actions(gap, B, STEPS)
    net = wa.hub8_network(B, history=history)
    env = VecPedNetEnv("hub8", n_envs=B, obs_mode=mode, normalize_obs=normalize, action_gap=gap, network=net, reward_mode=reward_mode)
    assert env.n_actions == 8 and env.n_obs == 8 * env.features_per_link
    for k in range(STEPS):
        obs, rew, *_ = env.step(acts[k])
        for r in replicas:
            so.assert_same_bits(obs[r], want[r][0][k], f"observation of replica {r} at env step {k}")
            so.assert_same_bits(rew[r], want[r][1][k], f"reward of replica {r} at env step {k}")
    if history == "full":
        e = net.engine()
        assert e.error_flags()[0] == 0
        for name in ALL_FIELDS:
            got = e.read_block(LINK_FIELDS[name][0], 0, STEPS * gap + 1)[:, :e.n_links, :]
            for r in replicas:
                so.assert_same_bits(got[:, :, r].T, want[r][2][name], f"{name} of replica {r}", "[link, t]")
    env.close()


MODES = [(m, n) for m in ("option1", "option2", "option3") for n in (False, True)] + [("option4", False), ("option5", False)]


@pytest.mark.parametrize("reward_mode", ["all", "reference"])
@pytest.mark.parametrize("gap", [1, 2])
@pytest.mark.parametrize("mode,normalize", MODES)
def test_hub8_observations_and_rewards_equal_the_restated_reference(mode, normalize, gap, reward_mode):
    """70 envs (a group of 64 and a group of 6), random actions in [-0.5, width + 0.5]: observations and rewards of replicas 0, 63, 64, 69
    at every env step, and their 13 link histories.  (option4 with normalisation: the reference raises an IndexError.)"""
    run_hub8(mode, normalize, gap, reward_mode, 70, (0, 63, 64, 69))


@pytest.mark.parametrize("plan,history,B,replicas", [("obs_launch", "full", 70, (0, 63, 64, 69)), ("default", "recent", 70, (0, 63, 64, 69)),
                                                     ("chains", "full", 320, (0, 127, 128, 255, 256, 319))])
def test_hub8_under_the_other_launch_plans(plan, history, B, replicas, monkeypatch):
    """option2 with the observations as a launch of their own, with recent history, and as two half-batch chains (256 + 64 envs: both
    chains and the last, partly filled segment)"""
    set_plan(monkeypatch, plan)
    run_hub8("option2", False, 2, "all", B, replicas, history=history)


def test_reward_means_are_summed_in_numpys_order():
    """The reward-mean replicas (a batch of 16 at its own replica offset, all of them checked, action_gap 1 and 2): 70 (replica, step)
    pairs in which the float32 reward differs between NumPy's summation order of the two means (pz_pednet_env.py:573-574; pairwise from 8
    values on) and a left-to-right sum -- 35 under each action gap (tests/test_wide_agents_host.py requires 5, one per gap)."""
    covered = {}
    for gap in (1, 2):
        acts, want_obs, want_rew, seq = wa.reward_models(gap)
        net = wa.hub8_network(wa.REWARD_B, replica_offset=wa.REWARD_OFFSET)
        env = VecPedNetEnv("hub8", n_envs=wa.REWARD_B, obs_mode="option2", action_gap=gap, network=net, reward_mode="all")
        telling = so.bits(want_rew) != so.bits(seq)
        covered[gap] = 0
        for k in range(wa.REWARD_STEPS):
            obs, rew, *_ = env.step(acts[k])
            so.assert_same_bits(obs, want_obs[k], f"action_gap {gap}: observations at env step {k}", "[replica, column]")
            so.assert_same_bits(rew, want_rew[k], f"action_gap {gap}: rewards at env step {k} ({int(telling[k].sum())} of them tell the orders apart)",
                                "[replica, agent]")
            covered[gap] += int(telling[k].sum())
        env.close()
    print(f"(replica, step) pairs whose reward tells the summation orders apart: {covered}")
    assert min(covered.values()) >= 1 and sum(covered.values()) >= 5, covered


# ------------------------------------------------------------------------------------------------------------ controllers on hub8
HUB_CHECKED = (0, 63, 64, 255, 256, 319)


@functools.lru_cache(maxsize=None)
def hub8_controlled(case):
    """The fixture's episode for the replicas HUB_CHECKED on the CPU: RlOracle stepped by one set of numpy agents per replica.
    {replica: (actions [n + 1, 8] float64, obs [n, 32], rewards [n, 1], episode sums [n, 1])}"""
    g = Golden(case)
    _, info = load(case)
    net = build_network(g)
    model = flatten_network(net)
    links = [net.links[(0, k)] for k in range(1, 9)]
    n = info["env_steps"]
    out = {}
    for r in HUB_CHECKED:
        o = RlOracle(net, model, wa.HUB_SPEC, "option2", False, 1, seed=g.seed, replica=g.replica + r)
        agent = host_agents(info, links_of=lambda aid: links)["gate_0"]
        obs = np.float32([x for l in links for x in (0, 0, 0, l.width)])
        ep = np.zeros(1, np.float32)
        acts, obs_l, rew_l, ep_l = [], [], [], []
        for _ in range(n):
            a = agent.take_action(obs, deterministic=True)
            acts.append(a.astype(np.float64))
            obs, rew = o.step(a)
            ep = ep + rew
            obs_l.append(obs), rew_l.append(rew), ep_l.append(ep)
        acts.append(agent.take_action(obs, deterministic=True).astype(np.float64))
        assert o.o.flags() == 0
        out[r] = tuple(np.array(x) for x in (acts, obs_l, rew_l, ep_l))
    net.close()
    return out


def stepwise(case, plan, monkeypatch):
    want = hub8_controlled(case)
    g, info, env = make_env(case, 320, monkeypatch, plan)
    env.set_controllers(device_agents(env, info))
    obs, _ = env.reset()
    n = info["env_steps"]
    for k in range(n + 1):
        acts = env.controller_actions()
        for r in HUB_CHECKED:
            so.assert_same_bits(acts[r], want[r][0][k], f"{plan}: actions of replica {r} before env step {k}")
        if k == n:
            break
        obs, rew, term = env.step_controlled(1)
        ep = env.episode_rewards()
        for r in HUB_CHECKED:
            so.assert_same_bits(obs[r], want[r][1][k], f"{plan}: observation of replica {r} at env step {k}")
            so.assert_same_bits(rew[r], want[r][2][k], f"{plan}: reward of replica {r} at env step {k}")
            so.assert_same_bits(ep[r], want[r][3][k], f"{plan}: episode sum of replica {r} at env step {k}")
    assert term
    final = (obs, rew, ep, acts)
    env.close()
    return final


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("case", ["ctrl_hub8_gate", "ctrl_hub8_gate0"])
def test_hub8_controllers_step_by_step_in_many_envs(case, plan, monkeypatch):
    """320 envs, one controlled env step per call: the next actions, observations, rewards and episode sums of replicas in both groups
    of the first chain's ends, in the second chain and in the last segment, against the reference's rule restated on the CPU oracle."""
    stepwise(case, plan, monkeypatch)


def test_hub8_whole_episode_in_one_call_ends_where_the_stepwise_one_does(monkeypatch):
    case = "ctrl_hub8_gate0"
    final = stepwise(case, "default", monkeypatch)
    g, info, env = make_env(case, 320)
    env.set_controllers(device_agents(env, info))
    env.reset()
    obs, rew, term = env.step_controlled()
    assert term
    for got, want, what in zip((obs, rew, env.episode_rewards(), env.controller_actions()), final, ("observations", "rewards", "episode sums", "actions")):
        so.assert_same_bits(got, want, what, "[replica, column]")
    env.close()


# ------------------------------------------------------------------------------------------------------------ separator windows
@pytest.mark.parametrize("B,plan", [(70, "default"), (320, "chains")])
@pytest.mark.parametrize("window", list(wa.WINDOWS) + [None])
def test_separator_windows_on_the_sparse_corridor(window, B, plan, monkeypatch):
    """long_corridor under the pulse train of wide_agents.corridor_demand, the separator controller with a moving average over `window`
    values (None: no smoothing), two episodes with a reset in between (the buffer carries across it): the action the device decided at
    every step against the host agent of each checked replica, fed the device's own observations -- and, in the first episode, the
    observed outflow against the CPU oracle's.  With the reverse term at 0 the action is (width * m) / m rounded to float32, which the
    last bits of the window's mean m almost never reach: what these cases pin is the content of the ring and its eviction (runs of zeros
    shorter and longer than the window, a lone value leaving a full window), not the pairwise order of the mean's sum."""
    set_plan(monkeypatch, plan)
    checked = wa.CORRIDOR_CHECKED[B]
    net = wa.corridor_network(B)
    so.upload(net, wa.corridor_demand(net, B))
    env = VecPedNetEnv("long_corridor", n_envs=B, obs_mode="option2", network=net)
    sid = env.possible_agents[0]
    env.set_controllers({sid: wa.separator_agent(window)})
    agents = {r: wa.separator_agent(window) for r in checked}
    flips = 0
    for episode in range(2):
        obs, _ = env.reset()
        for k in range(wa.CORRIDOR_STEPS):
            acts = env.controller_actions()
            for r in checked:
                a = agents[r].take_action(obs[r], deterministic=True)
                so.assert_same_bits(acts[r], a.astype(np.float64), f"window {window}: action of replica {r}, episode {episode}, before env step {k}")
                flips += a[0] == 2.0
            obs, rew, _ = env.step_controlled(1)
            if episode == 0:
                for r in checked:
                    assert obs[r, 1].tobytes() == wa.corridor_series(window, r)[0][k].tobytes(), (window, r, k)
    assert 0 < flips < 2 * wa.CORRIDOR_STEPS * len(checked)
    env.close()
