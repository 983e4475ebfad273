"""GPU tests of the rule-based controllers on the device (VecPedNetEnv.set_controllers / step_controlled, pedn_ctrl_*): every fixture
recorded with the reference's own agents bit for bit, for one env step by step and for whole episodes of many envs under each launch
plan of the batched RL step; the same episodes stepped through ``step`` with the numpy agents; no_control and metrics."""
import numpy as np
import pytest

from golden_util import ALL_FIELDS, Golden, build_network, step_digests
from pednstream_amd.evaluation import evaluate_agents
from pednstream_amd.metrics import network_metrics, replica
from pednstream_amd.network import LINK_FIELDS
from pednstream_amd.rl_env import VecPedNetEnv
from test_controllers_host import CTRL_CASES, host_agents, load

pytestmark = pytest.mark.gpu

# the launch plans of the batched RL step (tests/test_gpu_rl.py): default, observations as a launch of their own, two forked half-batch
# chains, actions applied by their own launch instead of inside node_kernel
PLANS = {"default": {}, "obs_launch": {"PEDN_FUSE_OBS": "0"}, "chains": {"PEDN_RL_CHAINS": "2", "PEDN_STREAM_PROBE": "0"},
         "no_fold": {"PEDN_RL_FOLD": "0"}}


def make_env(case, B, monkeypatch=None, plan="default", **kw):
    if monkeypatch is not None:
        for k, v in PLANS[plan].items():
            monkeypatch.setenv(k, v)
    g = Golden(case)
    _, info = load(case)
    rl = info["rl"]
    net = build_network(g, n_replicas=B, replica_offset=g.replica, rng_seed=g.seed)
    env = VecPedNetEnv(info["scenario"], n_envs=B, obs_mode=rl["obs_mode"], normalize_obs=rl["normalize"], action_gap=rl["action_gap"],
                       network=net, **kw)
    return g, info, env


def device_agents(env, info):
    return host_agents(info, links_of=env.agent_manager.get_gater_outgoing_links)


def field_problems(env, g, r=0):
    """The 13 per-link arrays of replica r against the fixture's digests at every time index."""
    e = env.network.engine()
    problems = []
    for name in ALL_FIELDS:
        mine = e.read_block(LINK_FIELDS[name][0], 0, g.steps)[:, :e.n_links, r].T
        bad = np.flatnonzero(step_digests(mine) != g.state("digest_" + name)[:g.steps])
        if len(bad):
            problems.append(f"{name}: differs at {len(bad)} time indices, first t={bad[0]}")
    return problems


def expected_actions(row):
    return np.asarray(row, dtype=np.float32).astype(np.float64)


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("case", CTRL_CASES)
def test_controlled_steps_reproduce_the_reference_fixture(case):
    """One env, one controlled env step per call: the reset observation and every step's observations, rewards, episode sums and next
    actions as the reference's agents produced them, and the histories of the (last) episode."""
    g, info, env = make_env(case, 1)
    z = g.z
    acts, obs_f, rew_f, ep_f, episode, reset_obs = (z["state_ctrl_" + k] for k in ("actions", "obs", "rewards", "episode_sums", "episode", "reset_obs"))
    env.set_controllers(device_agents(env, info))
    for k in range(len(acts)):
        if k == 0 or episode[k] != episode[k - 1]:
            obs, _ = env.reset()
            assert same(obs[0], reset_obs[episode[k]]), (k, "reset")
            assert (env.episode_rewards() == 0).all()
        assert same(env.controller_actions()[0], expected_actions(acts[k])), (k, env.controller_actions()[0], acts[k])
        obs, rew, term = env.step_controlled(1)
        assert same(obs[0], obs_f[k]), (k, obs[0], obs_f[k])
        assert same(rew[0], rew_f[k]), (k, rew[0], rew_f[k])
        assert same(env.episode_rewards()[0], ep_f[k]), (k, env.episode_rewards()[0], ep_f[k])
        assert term == (k == len(acts) - 1 or episode[k + 1] != episode[k])
    problems = field_problems(env, g)
    assert not problems, "\n".join(problems)
    env.close()


_host_loop = {}


def host_loop_episode(case, B, replicas=None):
    """The same episode for B envs through ``step`` with one set of numpy agents per env (the reference's evaluation loop, env by
    env): final observations, the last rewards and the float32 episode sums.  replicas: only these envs have agents (the others
    get no action; envs do not interact) and only their rows are returned, in this order."""
    if (case, B, replicas) not in _host_loop:
        g, info, env = make_env(case, B)
        chosen = range(B) if replicas is None else replicas
        agents = {r: device_agents(env, info) for r in chosen}
        ep = np.zeros((B, len(env.possible_agents)), np.float32)
        for e in range(info["episodes"]):
            obs, _ = env.reset()
            ep[:] = 0
            done = False
            while not done:
                row = np.full((B, env.n_actions), np.nan)
                for r in chosen:
                    for aid, ag in agents[r].items():
                        row[r, env.action_slices[aid]] = ag.take_action(obs[r, env.obs_slices[aid]], deterministic=True)
                obs, rew, done, _, _ = env.step(row)
                ep = ep + rew
        _host_loop[(case, B, replicas)] = tuple(x[list(chosen)] for x in (obs, rew, ep))
        env.close()
    return _host_loop[(case, B, replicas)]


@pytest.mark.parametrize("case,B,plan", [("ctrl_nine_gate3", B, p) for B in (1, 64, 320, 2048) for p in PLANS] +
                         [("ctrl_corridor_sep_smooth_2ep", B, "default") for B in (64, 2048)] +
                         [("ctrl_nine_gate3_g2n", 320, p) for p in ("default", "chains")] +
                         [("ctrl_small_gate08", 2048, "default"), ("ctrl_one_gate3", 320, "default")])
def test_whole_episodes_of_many_envs(case, B, plan, monkeypatch):
    """step_controlled() to the end of the episode in one call: replica 0 against the fixture, the first 64 replicas against the
    same episode stepped through ``step`` with the numpy agents -- and, beyond one group of 64, the replicas B // 2 and B // 2 + 63 (the
    second half-batch chain under PEDN_RL_CHAINS=2) and B - 1 (the last segment) against such a loop over just those replicas."""
    g, info, env = make_env(case, B, monkeypatch, plan)
    z = g.z
    env.set_controllers(device_agents(env, info))
    for e in range(info["episodes"]):
        env.reset()
        obs, rew, term = env.step_controlled()
        assert term
    assert same(obs[0], z["state_ctrl_obs"][-1]) and same(rew[0], z["state_ctrl_rewards"][-1])
    ep = env.episode_rewards()
    assert same(ep[0], z["state_ctrl_episode_sums"][-1])
    problems = field_problems(env, g)
    assert not problems, "\n".join(problems)
    n = min(B, 64)
    h_obs, h_rew, h_ep = host_loop_episode(case, 64)
    assert same(obs[:n], h_obs[:n]) and same(rew[:n], h_rew[:n]) and same(ep[:n], h_ep[:n])
    env.close()
    if B > 64:
        far = (B // 2, B // 2 + 63, B - 1)
        h_obs, h_rew, h_ep = host_loop_episode(case, B, far)
        assert same(obs[list(far)], h_obs) and same(rew[list(far)], h_rew) and same(ep[list(far)], h_ep)


def test_controlled_episode_in_stretches_and_with_recent_history():
    """Stretches of env steps (host waits in between) and recent-history mode give the one-call episode's results."""
    case = "ctrl_nine_gate3"
    out = []
    for history, stretch in (("full", None), ("full", 37), ("recent", 64)):
        g, info, env = make_env(case, 128, history=history)
        env.set_controllers(device_agents(env, info))
        env.reset()
        done = False
        while not done:
            left = (env.simulation_steps - env.sim_step + 1) // env.action_gap
            obs, rew, done = env.step_controlled(None if stretch is None else min(stretch, left))
        out.append((obs, rew, env.episode_rewards()))
        env.close()
    for o in out[1:]:
        assert all(same(a, b) for a, b in zip(out[0], o))


def test_no_control_equals_stepping_without_actions():
    g, info, env = make_env("ctrl_nine_gate3", 64)
    agents = device_agents(env, info)
    res = evaluate_agents(env, agents, no_control=True, verbose=False)
    got = env.episode_rewards()
    env.close()
    g, info, env = make_env("ctrl_nine_gate3", 64)
    env.reset()
    ep = np.zeros((64, len(env.possible_agents)), np.float32)
    done = False
    while not done:
        _, rew, done, _, _ = env.step(None)
        ep = ep + rew
    env.close()
    assert same(got, ep)
    cols = [env.possible_agents.index(a) for a in agents]
    assert res["total_reward"] == np.mean([sum(np.float32(x) for x in row) for row in ep[:, cols]])


def _equal(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_equal(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_evaluate_agents_with_metrics_equals_the_networks_metrics():
    g, info, env = make_env("ctrl_nine_gate3", 64, track_metrics=True)
    agents = device_agents(env, info)
    res = evaluate_agents(env, agents, verbose=False, num_runs=10, metrics=True)
    env.close()
    assert len(res["all_runs"]) == 10
    g, info, env = make_env("ctrl_nine_gate3", 64)
    env.set_controllers(device_agents(env, info))
    env.reset()
    env.step_controlled()
    ep = env.episode_rewards()
    m = network_metrics(env.network)
    env.close()
    for i, run in enumerate(res["all_runs"]):
        assert _equal(run["metrics"], replica(m, i)), i
        assert all(same(run["episode_rewards"][a], ep[i, env.possible_agents.index(a)]) for a in agents)


def test_set_controllers_checks_agents_against_the_env():
    from pednstream_amd.agents import RuleBasedGaterAgent, RuleBasedSeparatorAgent

    g, info, env = make_env("ctrl_nine_gate3", 1)
    aid = next(iter(info["controllers"]))
    other = [a for a in env.possible_agents if a != aid][0]
    with pytest.raises(ValueError, match="not the env's"):
        env.set_controllers({aid: RuleBasedGaterAgent(env.agent_manager.get_gater_outgoing_links(other), "option2")})
    with pytest.raises(ValueError, match="not a separator"):
        env.set_controllers({aid: RuleBasedSeparatorAgent(4)})
    with pytest.raises(ValueError, match="Unknown agent"):
        env.set_controllers({"gate_999": None})
    with pytest.raises(RuntimeError, match="set_controllers"):
        env.step_controlled()
    env.set_controllers({})
    with pytest.raises(RuntimeError, match="reset"):
        env.step_controlled()
    env.close()
    g, info, env = make_env("ctrl_corridor_sep_smooth", 1)
    sid = env.possible_agents[0]
    with pytest.raises(ValueError, match="buffer_size"):
        env.set_controllers({sid: RuleBasedSeparatorAgent(4, use_smoothing=True, buffer_size=33)})
    with pytest.raises(ValueError, match="width"):
        env.set_controllers({sid: RuleBasedSeparatorAgent(np.float32(4))})
    env.close()
