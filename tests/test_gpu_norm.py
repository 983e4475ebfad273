"""The running normalisation on the device (VecPedNetEnv.set_running_norm, pednstream_amd/csrc/pedn_norm.hpp) against the reference's
wrapper (goldens norm_*.npz, one env) and against the contract's numpy restatement (tests/norm_model.py, batches) -- bit for bit."""
import numpy as np
import pytest

from golden_util import DATA, Golden, build_network
from norm_model import NormModel
from pednstream_amd import NetworkEnvGenerator
from pednstream_amd.normalize import RunningNormalizeWrapper
from pednstream_amd.rl_env import MultiScenarioVecEnv, PedNetParallelEnv, VecPedNetEnv, _DeviceBuffer
from test_norm_contract import load_norm

pytestmark = pytest.mark.gpu

T_SHORT = 30


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def mixed_env(n_envs, obs_mode="option3", **kw):
    """long_corridor with its separator agent and two gater agents added (nodes 1 and 4), 30 steps long: both agent types, 4 + 4 x
    features_per_link observation columns (16, 24 or 32: one or two column tiles), an episode short enough to run to its terminated step."""
    gen = NetworkEnvGenerator(DATA)
    gen.network_data = gen.load_network_data("long_corridor")
    gen.config["params"]["controllers"]["nodes"] = [1, 4]
    gen.config["params"]["simulation_steps"] = T_SHORT
    np.random.seed(3)
    net = gen.create_network("long_corridor", verbose=False, n_replicas=n_envs, rng_seed=1)
    return VecPedNetEnv("long_corridor", n_envs=n_envs, obs_mode=obs_mode, network=net, reward_mode="all", **kw)


def tree_equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(tree_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(tree_equal(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def model_of(env, **kw):
    tracked, agent = env.norm_layout()
    return NormModel(env.n_envs, tracked, agent, len(env.possible_agents), **kw)


def stats_equal(a, b):
    assert set(a) == set(b)
    for aid in a["obs_rms"]:
        for k in ("mean", "var"):
            assert same(np.array(a["obs_rms"][aid][k]), np.array(b["obs_rms"][aid][k])), (aid, k)
        assert a["obs_rms"][aid]["count"] == b["obs_rms"][aid]["count"], aid
    if "ret_rms" in a:
        assert a["ret_rms"] == b["ret_rms"]


@pytest.mark.parametrize("flags", ["obs", "obsrew"])
@pytest.mark.parametrize("case", ["nine_opt3", "corridor_opt1"])
def test_single_env_wrapper_reproduces_the_reference_wrapper(case, flags):
    z, info = load_norm(case, flags)
    g = Golden("rl_" + case)
    rl = g.info["rl"]
    env = PedNetParallelEnv(g.info["scenario"], obs_mode=rl["obs_mode"], seed=g.seed,
                            network=build_network(g, n_replicas=1, replica_offset=g.replica, rng_seed=g.seed))
    env = RunningNormalizeWrapper(env, clip_obs=info["clip_obs"], clip_reward=info["clip_reward"], gamma=info["gamma"], **info["flags"])
    agents = env.possible_agents                      # (delegated)
    assert agents == info["agents"] and env.obs_builder.features_per_link == env._vec.features_per_link
    acts, raw_rew = g.state("rl_actions"), g.state("rl_rewards")
    obs, _ = env.reset()
    assert same(np.concatenate([obs[a] for a in agents]), z["reset_obs_n"])
    assert same(env._vec.raw_observations()[0], z["reset_obs"])
    for k in range(info["steps"]):
        if k == info["frozen_from"]:
            env.set_training(False)
        obs, rew, term, trunc, infos = env.step({a: acts[k, sl] for a, sl in env._vec.action_slices.items()})
        assert same(np.concatenate([obs[a] for a in agents]), z["obs_n"][k]), k
        assert same(np.float32([rew[a] for a in agents]), z["rew_n"][k].astype(np.float32)), k
        assert same(np.float32([infos[a]["true_reward"] for a in agents]), raw_rew[k]), k
        assert not any(term.values())
    s = env.get_normalization_stats()
    assert same(np.concatenate([s["obs_rms"][a]["mean"] for a in agents]), z["mean"])
    assert same(np.concatenate([s["obs_rms"][a]["var"] for a in agents]), z["var"])
    assert same(np.array([s["obs_rms"][a]["count"] for a in agents]), z["count"])
    if info["flags"]["norm_reward"]:
        assert same(np.array([s["ret_rms"][k] for k in ("mean", "var", "count")]), z["ret_rms"])
        assert env.ret_rms.var == z["ret_rms"][1]
    else:
        assert "ret_rms" not in s and env.ret_rms is None
    assert same(np.concatenate([env.obs_rms[a].mean for a in agents]), z["mean"])
    env.close()


@pytest.mark.parametrize("obs_mode", ["option1", "option3", "option5"])
@pytest.mark.parametrize("n_envs", [1, 2, 63, 64, 65, 130])
def test_batch_equals_the_numpy_contract(n_envs, obs_mode):
    env, twin = mixed_env(n_envs, obs_mode), mixed_env(n_envs, obs_mode)
    kw = dict(norm_obs=True, norm_reward=True, clip_obs=5.0, clip_reward=2.0, gamma=0.9)
    env.set_running_norm(**kw)
    model = model_of(env, **kw)
    tracked, _ = env.norm_layout()
    fpl = env.features_per_link
    assert env.n_obs == 4 + 4 * fpl and (~tracked).sum() == 4 and not tracked[4 + fpl - 1] and tracked[:4].all()
    rng = np.random.default_rng(n_envs)
    obs, _ = env.reset()
    raw, _ = twin.reset()
    model.reset()
    assert same(obs, model.observe(raw))
    for k in range(12):
        a = rng.uniform(-0.5, 4.5, size=(n_envs, env.n_actions))
        obs, rew, term, _, _ = env.step(a)
        raw, raw_rew, _, _, _ = twin.step(a)
        assert same(obs, model.observe(raw)), k
        assert same(rew, model.rewards(raw_rew, term)), k
        assert same(obs[:, ~tracked], raw[:, ~tracked])
        assert same(env.raw_observations(), raw) and same(env.true_rewards(), raw_rew)
    assert (raw_rew[:, 1:] != 0).any() and not same(obs, raw) and not same(rew, raw_rew)
    stats_equal(env.get_normalization_stats(), model.stats(env.possible_agents))
    env.close()
    twin.close()


def _policy(torch, n_actions):
    def policy(obs):      # depends on the NORMALISED observations it is handed
        return (obs[:, :n_actions].double().abs() * 0.7 + 0.5).remainder(3.0).contiguous()
    return policy


@pytest.mark.parametrize("n_envs", [2, 65])
def test_every_way_of_stepping_gives_the_same_bits_through_the_terminated_step(n_envs):
    torch = pytest.importorskip("torch")
    kw = dict(norm_obs=True, norm_reward=True, gamma=0.9)
    runs = {}
    for how in ("step", "device_sync", "device_async", "graph1", "graph3"):
        env = mixed_env(n_envs)
        env.set_running_norm(**kw)
        policy = _policy(torch, env.n_actions)
        log = []
        roll = env.capture(policy, steps_per_replay=int(how[-1])) if how.startswith("graph") else None
        env.reset()
        done = False
        while not done:
            if how == "step":
                o, r, done, _, _ = env.step(policy(env.device_views()[0]).cpu().numpy())
                log.append((o, r))
            elif roll is None:
                o, r, done = env.step_device(policy(env.device_views()[0]), sync=how == "device_sync")
                torch.cuda.synchronize()
                log.append((o.cpu().numpy(), r.cpu().numpy()))
            else:
                done = roll.step()
                torch.cuda.synchronize()
                o, r = env.device_views()
                log.append((o.cpu().numpy(), r.cpu().numpy()))
        assert env.sim_step == T_SHORT + 1
        if roll is not None:
            assert roll.replays == {"graph1": T_SHORT - 1, "graph3": (T_SHORT - 1) // 3}[how], (roll.replays, roll.eager_steps)
        runs[how] = (log, env.get_normalization_stats(), env.raw_observations(), env.true_rewards())
        env.close()
    ref_log, ref_stats, ref_raw, ref_true = runs["step"]
    assert len(ref_log) == T_SHORT
    for how, (log, stats, raw, true) in runs.items():
        stats_equal(stats, ref_stats)
        assert same(raw, ref_raw) and same(true, ref_true), how
        if how == "graph3":            # three policy steps per replay: only every graph's last rows are visible
            assert same(log[-1][0], ref_log[-1][0]) and same(log[-1][1], ref_log[-1][1])
        else:
            assert len(log) == T_SHORT
            for k, ((o, r), (o0, r0)) in enumerate(zip(log, ref_log)):
                assert same(o, o0) and same(r, r0), (how, k)
    # ... and what they all computed is the contract, the terminated step's discount included
    env, twin = mixed_env(n_envs), mixed_env(n_envs)
    env.set_running_norm(**kw)
    model = model_of(env, **kw)
    policy = _policy(torch, env.n_actions)
    obs, _ = env.reset()
    raw, _ = twin.reset()
    assert same(obs, model.observe(raw))
    term = False
    while not term:
        a = policy(env.device_views()[0]).cpu().numpy()
        obs, rew, term, _, _ = env.step(a)
        raw, raw_rew, _, _, _ = twin.step(a)
        assert same(obs, model.observe(raw)) and same(rew, model.rewards(raw_rew, term))
    stats_equal(env.get_normalization_stats(), model.stats(env.possible_agents))
    stats_equal(env.get_normalization_stats(), ref_stats)
    env.close()
    twin.close()


def test_training_switch_stats_round_trip_reset_and_recapture():
    torch = pytest.importorskip("torch")
    n_envs = 65
    kw = dict(norm_obs=True, norm_reward=True, gamma=0.9)
    env, twin = mixed_env(n_envs, track_metrics=True), mixed_env(n_envs, track_metrics=True)
    env.set_running_norm(**kw)
    model = model_of(env, **kw)
    n_agents = len(env.possible_agents)
    ret_view = lambda: torch.as_tensor(_DeviceBuffer(env.network.engine().rl_norm_device_ptr(5), (n_envs, n_agents), "<f8"),
                                       device="cuda").cpu().numpy()
    rng = np.random.default_rng(5)

    def steps(n):
        for _ in range(n):
            a = rng.uniform(0.0, 4.0, size=(n_envs, env.n_actions))
            obs, rew, term, _, _ = env.step(a)
            raw, raw_rew, _, _, _ = twin.step(a)
            assert same(obs, model.observe(raw)) and same(rew, model.rewards(raw_rew, term))

    obs, _ = env.reset()
    raw, _ = twin.reset()
    assert same(obs, model.observe(raw))
    steps(4)
    before = env.get_normalization_stats()
    env.set_training(False)                                   # frozen: rows are still normalised, statistics stay
    model.training = False
    steps(3)
    stats_equal(env.get_normalization_stats(), before)
    env.set_normalization_stats(env.get_normalization_stats())          # a fixed point
    stats_equal(env.get_normalization_stats(), before)
    env.set_training(True)
    model.training = True
    steps(2)
    assert env.get_normalization_stats()["obs_rms"]["sep_2_3"]["count"] == before["obs_rms"]["sep_2_3"]["count"] + 2 * n_envs
    assert ret_view().any() and same(ret_view(), model.ret)
    m_env, m_twin = env.episode_metrics(), twin.episode_metrics()          # works with track_metrics: the simulation is the twin's
    assert tree_equal(m_env, m_twin)
    mid = env.get_normalization_stats()
    obs, _ = env.reset()                                      # statistics survive a reset (and take in the reset observation), ret does not
    raw, _ = twin.reset()
    model.reset()
    assert not ret_view().any()
    assert same(obs, model.observe(raw))
    assert env.get_normalization_stats()["obs_rms"]["gate_1"]["count"] == mid["obs_rms"]["gate_1"]["count"] + n_envs
    steps(2)
    stats_equal(env.get_normalization_stats(), model.stats(env.possible_agents))
    # loading statistics: another env continues from them
    saved = env.get_normalization_stats()
    env.set_running_norm(None)
    obs_off, rew_off, *_ = env.step(None)
    raw, raw_rew, *_ = twin.step(None)
    assert same(obs_off, raw) and same(rew_off, raw_rew)     # off: the raw rows again
    with pytest.raises(RuntimeError):
        env.get_normalization_stats()
    env.set_running_norm(**kw)                               # on again: fresh statistics ...
    assert env.get_normalization_stats()["obs_rms"]["gate_4"]["count"] == 1e-4
    env.set_normalization_stats(saved)                       # ... until the saved ones are loaded
    stats_equal(env.get_normalization_stats(), saved)
    env.close()
    twin.close()

    # a captured rollout notices the switch: the graph is captured again and hands out the other buffers
    env = mixed_env(n_envs)
    policy = _policy(torch, env.n_actions)
    roll = env.capture(policy)
    env.reset()
    for _ in range(4):
        roll.step()
    assert roll.replays == 3 and roll.recaptures == 0
    raw_obs = env.raw_views()[0]
    assert env.device_views()[0].data_ptr() == raw_obs.data_ptr()
    env.set_running_norm(norm_obs=True)
    for _ in range(3):
        roll.step()
    torch.cuda.synchronize()
    assert roll.recaptures == 1 and roll.obs.data_ptr() == env.device_views()[0].data_ptr() != raw_obs.data_ptr()
    tracked = torch.as_tensor(env.norm_layout()[0], device="cuda")
    assert torch.equal(roll.obs[:, ~tracked], raw_obs[:, ~tracked]) and not torch.equal(roll.obs[:, tracked], raw_obs[:, tracked])
    env.set_running_norm(None)
    for _ in range(3):
        roll.step()
    assert roll.recaptures == 2 and roll.obs.data_ptr() == raw_obs.data_ptr()
    env.close()


def test_refused_combinations():
    env = mixed_env(2)
    env.set_running_norm()
    with pytest.raises(ValueError):
        env.set_controllers({})
    env.set_running_norm(None)
    env.set_controllers({})
    with pytest.raises(ValueError):
        env.set_running_norm()
    env.close()
    env = mixed_env(2)
    with pytest.raises(ValueError):
        env.set_running_norm(clip_obs=0.0)
    with pytest.raises(RuntimeError):
        env.set_training(False)
    env.close()
    multi = MultiScenarioVecEnv("long_corridor", n_envs=2, group_size=1, data_dir=DATA)
    with pytest.raises(ValueError):
        multi.set_running_norm()
    multi.groups[0].set_running_norm()
    multi.reset()
    with pytest.raises(RuntimeError):                         # the C entry point refuses too
        multi.step(np.full((2, multi.n_actions), 2.0))
    multi.close()
    with pytest.raises(TypeError):
        RunningNormalizeWrapper(object())
