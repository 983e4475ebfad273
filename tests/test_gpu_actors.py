"""The stacked actors on the device (pednstream_amd/policy.py, pednstream_amd/csrc/pedn_actor.hpp) against the contract's numpy
restatement (tests/actor_model.py): plain tensors, drawn noise, and as the captured policy of an env."""
import numpy as np
import pytest

import actor_model as am
from golden_util import DATA

pytestmark = pytest.mark.gpu

TABLES = {"one": ([(4, 1)], 0), "mixed": ([(4, 1), (56, 8), (6, 2)], 1), "five": ([(15, 3)] * 5, 0)}     # (obs_w, act_w), gap before agent 1
N_ENVS = (1, 3, 40, 65, 130)          # 40: not a multiple of the 32-env tile, more than one tile; 65, 130: a tile's first row and beyond
N_MAX = 130


def table(name):
    """agents [(obs0, obs_w, act0, act_w)], n_obs, n_actions; in "mixed" the second agent starts on an odd column."""
    widths, gap = TABLES[name]
    agents, o, a = [], 0, 0
    for i, (ow, aw) in enumerate(widths):
        o += gap if i == 1 else 0
        agents.append((o, ow, a, aw))
        o, a = o + ow, a + aw
    return agents, o, a


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    """bit-equal, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.where(nan, 0, bits(a)), np.where(nan, 0, bits(b)))


def within_ulps(a, b, n):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        return bool(np.all(nan | (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= n * am.ulp(b))))


def host(t):
    return t.detach().cpu().numpy()


def random_sd(rng, kind, obs_w, act_w, S, scale=2.0):
    from pednstream_amd.policy import tensor_shapes

    sd = {}
    for key, shape in tensor_shapes(kind, obs_w, act_w, S):
        fan = shape[-1] if len(shape) == 2 else 64
        v = rng.uniform(-1, 1, size=shape) * scale / np.sqrt(fan)
        if key == "ln.weight":
            v = 1 + 0.2 * rng.uniform(-1, 1, size=shape)
        sd[key] = v.astype(np.float32)
    return sd


_setups = {}


def setup(name, S, kind):
    """Parameters, a stack of N_MAX envs, noise and bounds of a case: drawn once, shared, never written."""
    key = (name, S, kind)
    if key not in _setups:
        agents, n_obs, n_actions = table(name)
        rng = np.random.default_rng(1000 * len(name) + 10 * S + (kind == "ppo"))
        sds = [random_sd(rng, kind, ow, aw, S) for (_, ow, _, aw) in agents]
        stack = (rng.standard_normal((N_MAX, S, n_obs)) * 2 + 1).astype(np.float32)
        noise = rng.standard_normal((N_MAX, n_actions)).astype(np.float32)
        low, high = np.zeros(n_actions, dtype=np.float32), rng.uniform(2, 6, size=n_actions).astype(np.float32)
        _setups[key] = (agents, n_obs, n_actions, sds, stack, noise, low, high)
    return _setups[key]


_models = {}


def model_forward(name, S, kind):
    """mu, z, std [N_MAX, n_actions] of the model, once per case"""
    key = (name, S, kind)
    if key not in _models:
        agents, n_obs, n_actions, sds, stack, *_ = setup(name, S, kind)
        out = [np.zeros((N_MAX, n_actions), dtype=np.float32) for _ in range(3)]
        for (o0, ow, a0, aw), sd in zip(agents, sds):
            for dst, v in zip(out, am.forward(kind, sd, stack[:, :, o0:o0 + ow])):
                dst[:, a0:a0 + aw] = v
        _models[key] = out
    return _models[key]


def make_actors(name, S, kind, n_envs, delta=True, **kw):
    from pednstream_amd.policy import StackedActors

    agents, n_obs, n_actions, sds, stack, noise, low, high = setup(name, S, kind)
    actors = StackedActors(kind, agents, low, high, n_envs, n_obs, n_actions, stack_size=S, delta_actions=delta, **kw)
    for i, sd in enumerate(sds):
        actors.load_state_dict(i, sd)
    return actors


def model_tail(name, S, kind, delta, mu, std, eps, stack, deterministic=False):
    """raw, actions of the model from the given mu / std / eps rows (all agents)"""
    agents, n_obs, n_actions, sds, _, _, low, high = setup(name, S, kind)
    raw, act = np.zeros(mu.shape, dtype=np.float32), np.zeros(mu.shape, dtype=np.float64)
    for (o0, ow, a0, aw) in agents:
        sl = slice(a0, a0 + aw)
        width = am.widths(stack[:, :, o0:o0 + ow], aw) if ow % aw == 0 else np.zeros((mu.shape[0], aw), dtype=np.float32)
        raw[:, sl], act[:, sl] = am.act_tail(kind, mu[:, sl], std[:, sl], eps[:, sl], width, low[sl], high[sl], delta_actions=delta,
                                             deterministic=deterministic)
    return raw, act


def model_actions(name, S, kind, delta, raw, stack):
    agents, _, _, _, _, _, low, high = setup(name, S, kind)
    act = np.zeros(raw.shape, dtype=np.float64)
    for (o0, ow, a0, aw) in agents:
        sl = slice(a0, a0 + aw)
        act[:, sl] = am.actions_of(raw[:, sl], am.widths(stack[:, :, o0:o0 + ow], aw), low[sl], high[sl], delta)
    return act


def check_outputs(name, S, kind, delta, n, actors, act, stack_rows, eps_in, want_mu, want_std, deterministic=False):
    out = {k: host(v) for k, v in actors.outputs.items()}
    act = host(act)
    assert same(out["mu"], want_mu), "mu"
    assert within_ulps(out["std"], want_std, 1), "std"
    assert same(out["eps"], eps_in), "eps"
    raw, _ = model_tail(name, S, kind, delta, out["mu"], out["std"], out["eps"], stack_rows, deterministic)
    if kind == "ppo":
        assert same(out["raw"], raw), "raw"
    else:
        assert within_ulps(out["raw"], raw, 2), "raw"
    assert same(act, model_actions(name, S, kind, delta, out["raw"], stack_rows)), "actions"
    return out, act


# ---------------------------------------------------------------------------------------------------- plain tensors
@pytest.mark.parametrize("delta", [True, False])
@pytest.mark.parametrize("kind", ["sac", "ppo"])
@pytest.mark.parametrize("S", [1, 4, 5])
@pytest.mark.parametrize("name", list(TABLES))
def test_kernel_equals_the_model(name, S, kind, delta):
    torch = pytest.importorskip("torch")
    agents, n_obs, n_actions, sds, stack, noise, low, high = setup(name, S, kind)
    mu, z, std = model_forward(name, S, kind)
    whole = None
    for n in N_ENVS:
        actors = make_actors(name, S, kind, n, delta)
        st = torch.as_tensor(stack[:n]).cuda()
        act = actors.act(st if not (S == 1 and n == 3) else st.view(n, n_obs), noise=torch.as_tensor(noise[:n]).cuda())
        assert act is actors.actions and act.dtype == torch.float64 and tuple(act.shape) == (n, n_actions)
        out, act = check_outputs(name, S, kind, delta, n, actors, act, stack[:n], noise[:n], mu[:n], std[:n])
        assert actors.draws() == 0                                     # supplied noise is no draw
        whole = (out, act) if n == N_MAX else whole
        if n == 3:                                                     # deterministic: eps = 0, raw from mu alone
            act = actors.act(st, deterministic=True)
            check_outputs(name, S, kind, delta, n, actors, act, stack[:n], np.zeros_like(noise[:n]), mu[:n], std[:n], deterministic=True)
    # batch independence: env 77 of the 130-env launch alone, as env 0 of a launch of one
    e = 77
    actors = make_actors(name, S, kind, 1, delta)
    act = host(actors.act(torch.as_tensor(stack[e:e + 1]).cuda(), noise=torch.as_tensor(noise[e:e + 1]).cuda()))
    assert same(act, whole[1][e:e + 1])
    for k, v in actors.outputs.items():
        assert same(host(v), whole[0][k][e:e + 1]), k


@pytest.mark.parametrize("kind", ["sac", "ppo"])
def test_awkward_inputs_stay_in_their_row(kind):
    torch = pytest.importorskip("torch")
    name, S, n = "mixed", 4, 40
    agents, n_obs, n_actions, sds, stack, noise, low, high = setup(name, S, kind)
    x = stack[:n].copy()
    x[3, 1, :] = np.nan                                                # a NaN frame of env 3
    x[5, :, ::3] = -0.0
    x[7, :, ::2] = np.float32(1e-41)                                   # subnormals
    x[8, :, :] = np.float32(-3e-45)
    x[35, 2, 7] = np.nan                                               # one NaN column (agent 1's) in the second tile
    mu, std = np.zeros((n, n_actions), dtype=np.float32), np.zeros((n, n_actions), dtype=np.float32)
    for (o0, ow, a0, aw), sd in zip(agents, sds):
        mu[:, a0:a0 + aw], _, std[:, a0:a0 + aw] = am.forward(kind, sd, x[:, :, o0:o0 + ow])
    actors = make_actors(name, S, kind, n)
    act = actors.act(torch.as_tensor(x).cuda(), noise=torch.as_tensor(noise[:n]).cuda())
    out, act = check_outputs(name, S, kind, True, n, actors, act, x, noise[:n], mu, std)
    nan_rows = np.isnan(act).any(axis=1)
    assert nan_rows.tolist() == [e in (3, 35) for e in range(n)]
    assert np.isnan(act[3]).all() and np.isnan(out["mu"][3]).all()
    a1 = slice(agents[1][2], agents[1][2] + agents[1][3])
    assert np.isnan(act[35, a1]).all() and not np.isnan(np.delete(act[35], np.r_[a1])).any()


# ---------------------------------------------------------------------------------------------------- drawn noise
def test_drawn_noise_is_the_contracts():
    torch = pytest.importorskip("torch")
    name, S, kind, n = "mixed", 4, "sac", 130
    agents, n_obs, n_actions, sds, stack, noise, low, high = setup(name, S, kind)
    mu, z, std = model_forward(name, S, kind)
    seed = 0x5EED_0000_0000_0072
    st = torch.as_tensor(stack).cuda()
    g, c = np.arange(n)[:, None], np.arange(n_actions)[None, :]
    actors = make_actors(name, S, kind, n, seed=seed)
    runs = []
    for d in (0, 1):
        act = actors.act(st)
        want = am.noise(seed, g, c, d)
        eps = host(actors.outputs["eps"])
        tol = 2.0 ** -23 * np.maximum(np.abs(want.astype(np.float64)), 2.0 ** -10)
        assert np.all(np.abs(eps.astype(np.float64) - want) <= tol), d
        check_outputs(name, S, kind, True, n, actors, act, stack, eps, mu, std)
        runs.append(eps)
    assert actors.draws() == 2 and not same(runs[0], runs[1])
    again = make_actors(name, S, kind, n, seed=seed)
    again.act(st)
    assert same(host(again.outputs["eps"]), runs[0])
    other = make_actors(name, S, kind, n, seed=seed + 1)
    other.act(st)
    assert not np.any(bits(host(other.outputs["eps"])) == bits(runs[0]))
    # global env indices: rows 64.. of the launch above are a launch of 66 envs at replica_offset 64
    tail = make_actors(name, S, kind, n - 64, seed=seed, replica_offset=64)
    act = host(tail.act(torch.as_tensor(stack[64:]).cuda()))
    assert same(host(tail.outputs["eps"]), runs[0][64:])
    again.act(st, deterministic=True)                                  # no draw
    assert again.draws() == 1 and not host(again.outputs["eps"]).any()


# ---------------------------------------------------------------------------------------------------- with an env
def nine(n_envs):
    from pednstream_amd.rl_env import VecPedNetEnv

    np.random.seed(3)                  # (the scenario's demand is drawn from numpy's global stream when the network is built)
    return VecPedNetEnv("nine_intersections", n_envs=n_envs, obs_mode="option3", data_dir=DATA, seed=5)


def corridor(n_envs):
    from pednstream_amd.rl_env import VecPedNetEnv

    np.random.seed(3)
    return VecPedNetEnv("long_corridor", n_envs=n_envs, obs_mode="option3", data_dir=DATA, seed=5)


def env_actors(env, kind, S, seed=11, rng_seed=3):
    rng = np.random.default_rng(rng_seed)
    actors = env.stacked_actors(kind=kind, stack_size=S, seed=seed)
    sds = {}
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        sds[aid] = random_sd(rng, kind, o.stop - o.start, a.stop - a.start, S, scale=1.0)
        actors.load_state_dict(aid, sds[aid])
    return actors, sds


def rollout(torch, make_env, kind, how, steps=12, S=4):
    env = make_env()
    buf = env.replay_store(steps + 2, stack_size=S, seed=1)
    actors, _ = env_actors(env, kind, S)
    log = []
    keep = lambda obs, rew: log.append((host(actors.actions.clone()), host(obs.clone()), host(rew.clone()), host(actors.outputs["eps"].clone())))
    env.reset()
    buf.begin()
    roll = None
    if how == "graph":
        roll = env.capture(lambda obs: actors.act(buf.stacked_obs()), on_step=lambda obs, rew: buf.push(actors.actions))
        for _ in range(steps):
            roll.step()
            torch.cuda.synchronize()
            keep(*env.device_views())
        assert roll.replays == steps - 1 and roll.eager_steps == 1 and roll.recaptures == 0
    else:
        for _ in range(steps):
            a = actors.act(buf.stacked_obs())
            obs, rew, _ = env.step_device(a, sync=True)
            buf.push(a)
            torch.cuda.synchronize()
            keep(obs, rew)
    assert actors.draws() == steps
    env.close()
    return log


@pytest.mark.parametrize("make_env,n_envs,kind", [(nine, 3, "sac"), (nine, 65, "sac"), (nine, 3, "ppo"), (corridor, 3, "sac"), (corridor, 3, "ppo")])
def test_a_replayed_rollout_equals_an_eager_one(make_env, n_envs, kind):
    torch = pytest.importorskip("torch")
    eager = rollout(torch, lambda: make_env(n_envs), kind, "eager")
    graph = rollout(torch, lambda: make_env(n_envs), kind, "graph")
    assert len(eager) == len(graph) == 12
    for t, (a, b) in enumerate(zip(eager, graph)):
        for x, y, what in zip(a, b, ("actions", "observations", "rewards", "eps")):
            assert same(x, y), (t, what)
    assert not same(eager[3][3], eager[4][3])                                             # every step draws anew
    if make_env is nine:          # the env moves (the corridor is still empty after 12 steps, its separator's action sits on a bound)
        assert not same(eager[0][1], eager[11][1]) and not same(eager[0][0], eager[5][0])
    assert np.isfinite(eager[-1][0]).all()


def mixed(n_envs):
    from test_gpu_norm import mixed_env

    return mixed_env(n_envs)          # long_corridor with its separator and two gaters, busy from the first steps


@pytest.mark.parametrize("make_env", [nine, mixed])
def test_delta_actions_read_the_widths_the_reference_reads(make_env):
    """Under the running normalisation the last feature of a gater's links (the gate width) is handed out as it is, so the delta is added
    to the un-normalised width; a separator's four features are all normalised, and like the reference's loop the kernel adds the delta to
    the normalised last one."""
    torch = pytest.importorskip("torch")
    env = make_env(3)
    env.set_running_norm(norm_obs=True)
    S = 4
    buf = env.replay_store(8, stack_size=S, seed=1)
    actors, sds = env_actors(env, "sac", S)
    env.reset()
    buf.begin()
    for _ in range(10):
        a = actors.act(buf.stacked_obs())
        env.step_device(a, sync=True)
        buf.push(a)
    act = host(actors.act(buf.stacked_obs()))
    torch.cuda.synchronize()
    obs, raw_obs, out = host(env.device_views()[0]), host(env.raw_views()[0]), {k: host(v) for k, v in actors.outputs.items()}
    assert same(host(buf.stacked_obs())[:, -1], obs) and not same(obs, raw_obs)
    for aid, ty in zip(env.possible_agents, env._types):
        o, sl = env.obs_slices[aid], env.action_slices[aid]
        aw = sl.stop - sl.start
        src = raw_obs if ty == 1 else obs
        width = src[:, o].reshape(3, aw, -1)[:, :, -1]
        assert same(act[:, sl], am.actions_of(out["raw"][:, sl], width, env.action_low[sl], env.action_high[sl], True)), aid
    env.close()


@pytest.mark.parametrize("kind", ["sac", "ppo"])
def test_bind_makes_the_optimiser_update_what_the_kernel_reads(kind):
    torch = pytest.importorskip("torch")
    from pednstream_amd.policy import make_module

    name, S, n = "mixed", 4, 40
    agents, n_obs, n_actions, sds, stack, noise, low, high = setup(name, S, kind)
    actors = make_actors(name, S, kind, n)
    torch.manual_seed(2)
    st = torch.as_tensor(stack[:n]).cuda()
    mods = []
    for i, (o0, ow, a0, aw) in enumerate(agents):
        m = make_module(kind, ow, aw, S).cuda()
        actors.bind(i, m)
        views = actors.parameters(i)
        assert all(p.data_ptr() == views[k].data_ptr() for k, p in m.named_parameters())
        mods.append(m)
    opt = torch.optim.Adam([p for m in mods for p in m.parameters()], lr=1e-2)
    for i, (o0, ow, a0, aw) in enumerate(agents):
        mu, std = mods[i](st[:, :, o0:o0 + ow])
        # the module's float32 forward is the kernel's up to the summation order
        actors.act(st, deterministic=True)
        assert torch.allclose(mu, actors.outputs["mu"][:, a0:a0 + aw], rtol=1e-4, atol=1e-5)
        assert torch.allclose(std, actors.outputs["std"][:, a0:a0 + aw], rtol=1e-4, atol=1e-5)
        (mu.square().sum() + std.sum()).backward()
    before = host(actors.outputs["mu"]).copy()
    opt.step()
    act = actors.act(st, noise=torch.as_tensor(noise[:n]).cuda())
    want_mu, want_std = np.zeros((n, n_actions), dtype=np.float32), np.zeros((n, n_actions), dtype=np.float32)
    for i, (m, (o0, ow, a0, aw)) in enumerate(zip(mods, agents)):
        views = actors.parameters(i)
        assert all(p.data_ptr() == views[k].data_ptr() for k, p in m.named_parameters())       # the step was in place
        sd = {k: host(v) for k, v in m.state_dict().items()}
        want_mu[:, a0:a0 + aw], _, want_std[:, a0:a0 + aw] = am.forward(kind, sd, stack[:n, :, o0:o0 + ow])
    check_outputs(name, S, kind, True, n, actors, act, stack[:n], noise[:n], want_mu, want_std)
    assert not same(host(actors.outputs["mu"]), before)


def test_refusals_on_the_device():
    torch = pytest.importorskip("torch")
    name, S, kind, n = "one", 4, "sac", 3
    agents, n_obs, n_actions, sds, stack, noise, low, high = setup(name, S, kind)
    from pednstream_amd.policy import StackedActors

    actors = StackedActors(kind, agents, low, high, n, n_obs, n_actions, stack_size=S)
    st = torch.as_tensor(stack[:n]).cuda()
    with pytest.raises(ValueError, match="no parameters were loaded"):
        actors.act(st)
    actors.load_state_dict(0, sds[0])
    for bad in (st[:2], st.double(), st.transpose(1, 2), st.view(n, S * n_obs)):
        with pytest.raises(ValueError, match="stack must"):
            actors.act(bad)
    with pytest.raises(ValueError, match="noise must"):
        actors.act(st, noise=torch.zeros(n, n_actions))
    with pytest.raises(ValueError, match="Unknown agent"):
        actors.bind(5, torch.nn.Linear(2, 2))
    actors.act(st)
