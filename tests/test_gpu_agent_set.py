"""A second ``pedn_rl_configure`` on a LIVE engine: the running normalisation, the rollout store and the replay store belong to the agent
set and go with it, and the engine then behaves, bit for bit, like a fresh one that was given the second agent set directly -- the path on
which the stores' drops, their row sources and the subsystems' flags meet (pednstream_amd/csrc/pedn_hip.hip: pedn_rl_configure)."""
import numpy as np
import pytest

from golden_util import DATA
from pednstream_amd import NetworkEnvGenerator
from pednstream_amd.rl_env import VecPedNetEnv

pytestmark = pytest.mark.gpu

N_ENVS = 128
T_SHORT = 30
SEED = 0x5EED_0000_0000_0071
NOT_CONFIGURED = "pedn_%s_configure has not been called"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(t):
    return t.detach().cpu().numpy()


def network():
    """nine_intersections (gaters at nodes 3, 4, 7) with a separator agent added on corridor 1-2, 30 steps long."""
    gen = NetworkEnvGenerator(DATA)
    gen.network_data = gen.load_network_data("nine_intersections")
    gen.config["params"]["controllers"]["links"] = ["1-2"]
    gen.config["params"]["simulation_steps"] = T_SHORT
    np.random.seed(3)
    return gen.create_network("nine_intersections", verbose=False, n_replicas=N_ENVS, rng_seed=5)


def env_of(net):
    """Configures the engine of ``net`` with the agents the network names NOW (on a live engine: a second pedn_rl_configure)."""
    return VecPedNetEnv("nine_intersections", n_envs=N_ENVS, obs_mode="option3", network=net, reward_mode="all")


def drive(torch, env, steps):
    """Normalisation on, both stores configured, ``steps`` env steps from a reset, recorded and pushed; everything a learner would see."""
    env.set_running_norm(norm_obs=True, norm_reward=True)
    ro = env.rollout_store(capacity=steps)
    rp = env.replay_store(steps, stack_size=2, seed=SEED)
    out = {}
    out["obs0"], _ = env.reset()
    ro.begin()
    rp.begin()
    for k in range(steps):
        a = (env.device_views()[0][:, :env.n_actions].double().abs() * 0.7 + 0.5).remainder(3.0).contiguous()
        obs, rew, _ = env.step_device(a)
        ro.record(a)
        rp.push(a)
        torch.cuda.synchronize()
        out[f"obs{k + 1}"], out[f"rew{k + 1}"] = host(obs.clone()), host(rew.clone())
        out[f"raw_obs{k + 1}"], out[f"raw_rew{k + 1}"] = (host(x.clone()) for x in env.raw_views())
    assert ro.finish() == steps and not ro.overflow
    for k, v in ro.views().items():
        out["rollout_" + k] = host(v)
    return out, ro, rp


def test_second_agent_set_on_a_live_engine_equals_a_fresh_engine():
    torch = pytest.importorskip("torch")
    net = network()
    first = env_of(net)
    types = list(first._types)
    assert 0 in types and 1 in types, types           # a separator and gaters
    eng = net.engine()
    _, ro, rp = drive(torch, first, 3)
    assert eng.rl_norm_device_ptr(0) and eng.rollout_device_ptr(0) and eng.replay_device_ptr(0)
    sig = eng.rl_clock_signature()

    net.controller_links = []                          # the gaters only
    live = env_of(net)
    assert net.engine() is eng and list(live._types) == [1] * (len(types) - 1)
    assert (live.n_actions, live.n_obs) != (first.n_actions, first.n_obs)
    # the stores went with the first agent set ...
    for name, begin in (("rollout", eng._lib.pedn_rollout_begin), ("replay", eng._lib.pedn_replay_begin)):
        assert begin(eng._h) == -1                     # PEDN_E_ARG
        assert eng._lib.pedn_last_error(eng._h).decode() == NOT_CONFIGURED % name
    assert not eng.rollout_device_ptr(0) and not eng.replay_device_ptr(0) and not eng.rl_norm_device_ptr(0)
    # ... and so did the normalisation: the fetches hand out the raw rows
    live.reset()
    for got, raw in zip(eng.rl_fetch(), eng.rl_fetch_raw()):
        assert same(got, raw)
    assert eng.rl_fetch()[0].any()
    assert eng.rl_clock_signature() != sig

    fresh_net = network()
    fresh_net.controller_links = []
    fresh = env_of(fresh_net)
    assert list(fresh._types) == list(live._types) and (fresh.n_actions, fresh.n_obs) == (live.n_actions, live.n_obs)
    want, _, rp_fresh = drive(torch, fresh, 5)
    got, _, rp_live = drive(torch, live, 5)
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), k
    assert want["obs5"].any() and want["rew5"].any() and not same(want["obs5"], want["raw_obs5"])
    # a minibatch with given indices.  (The first sample call of a batch size allocates and zeroes its output tensors on torch's current
    # stream; with the default stream current the gather runs on the engine's own stream, which that fill does not order: so every
    # store samples once and is waited for before the calls that count.)
    rp_fresh.sample(batch_size=96)
    torch.cuda.synchronize()
    idx = rp_fresh.sample(batch_size=96)[5]
    torch.cuda.synchronize()
    idx = idx.clone()
    rp_live.sample(indices=idx)
    torch.cuda.synchronize()
    out_live, out_fresh = rp_live.sample(indices=idx), rp_fresh.sample(indices=idx)
    torch.cuda.synchronize()
    for a, b in zip(out_live[:5], out_fresh[:5]):
        assert same(host(a), host(b))
    assert host(out_live[0]).any() and len(np.unique(host(idx), axis=0)) > 1
    a, b = rp_live.state(), rp_fresh.state()            # (raises if a sample was refused)
    assert all(a[k] == b[k] for k in ("head", "steps", "size_rows", "first"))
    # the statistics of the running normalisation
    for a, b in zip(eng.rl_norm_get_stats(), fresh_net.engine().rl_norm_get_stats()):
        assert same(a, b)
    assert eng.rl_clock_signature() != sig
    live.close()
    fresh.close()
