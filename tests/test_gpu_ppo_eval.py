"""PPO's rollout evaluation on the device (pednstream_amd/ppo.py, pednstream_amd/csrc/pedn_ppo.hpp) against the contract's numpy
restatement (tests/ppo_eval_model.py): plain tensors, the acting kernel, bound torch modules, a captured launch and an env's store.  The
checks are staged like test_gpu_sac_targets.check: what the contract evaluates in float32 (values, mu) is compared bit for bit, std within
1 ulp (its softplus is a float64 evaluation rounded once), and the log-probability within 2 ulps of the model's tail fed the kernel's own
mu and std."""
import numpy as np
import pytest

import actor_model as am
import ppo_eval_model as pm
import rollout_model as rm
from test_gpu_actors import env_actors, host, nine, random_sd, same
from test_gpu_sac_targets import table, within_ulps

pytestmark = pytest.mark.gpu

# (obs_w, act_w) per agent, gap before agent 1: test_gpu_sac_targets.TABLES.  With S in (1, 4, 5) the first layer's K1 = S * obs_w covers
# 4 .. 30 (less than a chunk of 32), 100 (no multiple of 32), 160, 200, 224 and 280
NAMES = ("one", "wide", "mixed50", "mixed")
TILE = 32
# T < S for S in (4, 5): every stack clamped; 9 rows: one tile that crosses time rows; 40 rows: a partial last tile; 70: more than two tiles
SHAPES = ((1, 1), (2, 3), (7, 5), (13, 5))
T_MAX, N_MAX = 13, 5
MIN_STD, MAX_STD = 1e-3, 10.0
F = np.float32


def random_value(rng, obs_w, S, scale=2.0):
    from pednstream_amd.ppo import value_tensor_shapes

    sd = {}
    for key, shape in value_tensor_shapes(obs_w, S):
        fan = shape[-1] if len(shape) == 2 else 64
        sd[key] = (rng.uniform(-1, 1, size=shape) * scale / np.sqrt(fan)).astype(F)
    return sd


_setups = {}


def setup(name, S):
    """Parameters, the observations and actions of a (T_MAX, N_MAX) rollout and the model's outputs for it: made once, shared, never
    written.  A row's numbers depend on its own frames only, so the model of a smaller (T, N) is the corner [:T + 1, :N] of this one."""
    key = (name, S)
    if key not in _setups:
        agents, n_obs, n_actions = table(name)
        rng = np.random.default_rng(3000 * len(name) + 10 * S)
        actors = [random_sd(rng, "ppo", ow, aw, S) for (_, ow, _, aw) in agents]
        values = [random_value(rng, ow, S) for (_, ow, _, _) in agents]
        obs = (rng.standard_normal((T_MAX + 1, N_MAX, n_obs)) * 2 + 1).astype(F)
        actions = (rng.standard_normal((T_MAX, N_MAX, n_actions)) * 1.5).astype(F)
        c = dict(agents=agents, n_obs=n_obs, n_actions=n_actions, actors=actors, values=values, obs=obs, actions=actions)
        c["model"] = pm.evaluate(agents, actors, values, obs, actions, S, MIN_STD, MAX_STD)
        _setups[key] = c
    return _setups[key]


def make(name, S, n_envs=1, load=True, min_std=MIN_STD, max_std=MAX_STD):
    pytest.importorskip("torch")
    from pednstream_amd.policy import StackedActors
    from pednstream_amd.ppo import PpoTargets

    c = setup(name, S)
    low, high = np.zeros(c["n_actions"], dtype=F), np.full(c["n_actions"], 4.0, dtype=F)
    actors = StackedActors("ppo", c["agents"], low, high, n_envs, c["n_obs"], c["n_actions"], stack_size=S, delta_actions=False, min_std=min_std,
                           max_std=max_std)
    ppo = PpoTargets(actors)
    if load:
        for i in range(len(c["agents"])):
            actors.load_state_dict(i, c["actors"][i])
            ppo.load_state_dict(i, c["values"][i])
    return ppo


def run(torch, ppo, obs, actions, **kw):
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()
    out = ppo.evaluate(dev(obs), dev(actions), want_mu_std=True, **kw)
    assert set(out) == {"values", "old_log_probs", "mu", "std"}
    return {k: host(v) for k, v in out.items()}


def check(out, want, actions):
    """The staged comparison of one launch's outputs with the model's (want) for the same rows."""
    for k in ("values", "mu", "std", "old_log_probs"):
        assert out[k].dtype == F and out[k].shape == want[k].shape, k
    assert same(out["values"], want["values"]), "values"
    assert same(out["mu"], want["mu"]), "mu"
    assert within_ulps(out["std"], want["std"], 1), "std"
    assert within_ulps(out["old_log_probs"], pm.log_prob(np.asarray(actions).astype(F), out["mu"], out["std"]), 2), "old_log_probs"


def corner(model, T, N):
    return {k: v[:T + (k == "values"), :N] for k, v in model.items()}


# ---------------------------------------------------------------------------------------------------- plain tensors
@pytest.mark.parametrize("S", [1, 4, 5])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_model(name, S):
    torch = pytest.importorskip("torch")
    c = setup(name, S)
    ppo = make(name, S)
    for T, N in SHAPES:
        obs, actions = c["obs"][:T + 1, :N], c["actions"][:T, :N]
        out = run(torch, ppo, obs, actions)
        check(out, corner(c["model"], T, N), actions)
    assert np.isfinite(out["old_log_probs"]).all() and np.isfinite(out["values"]).all()
    # allocated once per (T, N); without mu / std nothing but values and old_log_probs comes back
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()
    first = ppo.evaluate(dev(c["obs"][:3, :3]), dev(c["actions"][:2, :3]))
    again = ppo.evaluate(dev(c["obs"][:3, :3]), dev(c["actions"][:2, :3]))
    assert set(first) == {"values", "old_log_probs"} and all(first[k].data_ptr() == again[k].data_ptr() for k in first)


def test_both_std_bounds_are_hit():
    torch = pytest.importorskip("torch")
    name, S, lo, hi = "mixed", 4, 0.4, 1.2
    c = setup(name, S)
    want = pm.evaluate(c["agents"], c["actors"], c["values"], c["obs"], c["actions"], S, lo, hi)
    assert (want["std"] == F(lo)).any() and (want["std"] == F(hi)).any() and ((want["std"] > F(lo)) & (want["std"] < F(hi))).any()
    out = run(torch, make(name, S, min_std=lo, max_std=hi), c["obs"], c["actions"])
    check(out, want, c["actions"])
    assert (out["std"] == F(lo)).any() and (out["std"] == F(hi)).any()


def test_the_acting_kernel_computes_the_same_mu_and_std():
    torch = pytest.importorskip("torch")
    name, S, T, N = "mixed", 5, T_MAX, N_MAX
    c = setup(name, S)
    ppo = make(name, S, n_envs=T * N)
    out = run(torch, ppo, c["obs"], c["actions"])
    stack = pm.stacks(c["obs"], S)[:T].reshape(T * N, S, c["n_obs"])                  # the stack of every row, as ReplayStore.stacked_obs() hands it out
    ppo.actors.act(torch.as_tensor(stack).cuda(), deterministic=True)
    acted = {k: host(v).reshape(T, N, -1) for k, v in ppo.actors.outputs.items()}
    assert same(acted["mu"], out["mu"]) and same(acted["std"], out["std"])


def test_a_row_depends_on_its_own_frames_and_action_only():
    torch = pytest.importorskip("torch")
    name, S, T, N = "mixed", 4, T_MAX, N_MAX
    c = setup(name, S)
    ppo = make(name, S)
    whole = run(torch, ppo, c["obs"], c["actions"])
    as64 = run(torch, ppo, c["obs"], c["actions"].astype(np.float64))                   # float64 actions are read as (float)x
    for k in whole:
        assert same(whole[k], as64[k]), k
    filler = np.full((1, c["n_obs"]), 7.0, dtype=F)
    for t, e in ((0, 0), (2, 3), (7, 4), (12, 1), (13, 2)):
        # a 1-env rollout of the row's own S frames and one more: its row S - 1 has exactly these frames
        frames = c["obs"][pm.stack_times(T, S)[t], e]
        obs1 = np.concatenate([frames, filler])[:, None, :]
        act1 = np.zeros((S, 1, c["n_actions"]), dtype=F)
        if t < T:
            act1[S - 1, 0] = c["actions"][t, e]
        one = run(torch, ppo, obs1, act1)
        assert same(one["values"][S - 1, 0], whole["values"][t, e]), (t, e)
        if t < T:
            for k in ("mu", "std", "old_log_probs"):
                assert same(one[k][S - 1, 0], whole[k][t, e]), (k, t, e)


def test_awkward_values_change_the_rows_that_hold_them_and_nothing_else():
    torch = pytest.importorskip("torch")
    name, S, T, N = "mixed", 4, T_MAX, N_MAX
    c = setup(name, S)
    ppo = make(name, S)
    clean = run(torch, ppo, c["obs"], c["actions"])
    obs = c["obs"].copy()
    t0, e0 = 3, 2
    obs[t0, e0, 0::4] = np.nan                                           # every agent's columns hold some of each
    obs[t0, e0, 1::4] = np.inf
    obs[t0, e0, 2::4] = -np.inf
    obs[t0, e0, 3::4] = -0.0
    out = run(torch, ppo, obs, c["actions"])
    check(out, pm.evaluate(c["agents"], c["actors"], c["values"], obs, c["actions"], S, MIN_STD, MAX_STD), c["actions"])
    held = {(t, e0) for t in range(t0, t0 + S)}                          # the S rows of that env whose stacks hold the frame
    for k, v in out.items():
        for t in range(v.shape[0]):
            for e in range(N):
                if (t, e) in held:
                    assert np.isnan(v[t, e]).all(), (k, t, e)
                else:
                    assert same(v[t, e], clean[k][t, e]), (k, t, e)
    assert np.isfinite(clean["values"]).all() and np.isfinite(clean["old_log_probs"]).all()


# ---------------------------------------------------------------------------------------------------- bound modules
def test_bind_makes_the_optimiser_update_what_the_next_launch_reads():
    torch = pytest.importorskip("torch")
    from pednstream_amd.ppo import make_value_module

    name, S, T, N = "mixed50", 4, 2, 3
    c = setup(name, S)
    agents = c["agents"]
    ppo = make(name, S)
    torch.manual_seed(4)
    mods = [ppo.bind(i, make_value_module(ow, S).cuda()) for i, (_, ow, _, _) in enumerate(agents)]
    for i, m in enumerate(mods):
        views = ppo.parameters(i)
        assert all(p.data_ptr() == views[k].data_ptr() for k, p in m.named_parameters())
    pad = np.ones(ppo.pack_size, dtype=bool)
    for cur in ppo.offsets:
        for at, shape in cur.values():
            pad[at:at + int(np.prod(shape))] = False
    assert pad.sum() == 3 * len(agents) and ppo.pack_size % 4 == 0 and all(at % 4 == 0 for at in ppo.value_table)
    obs, actions = c["obs"][:T + 1, :N], c["actions"][:T, :N]

    def compare():
        out = run(torch, ppo, obs, actions)
        sds = [{k: host(v) for k, v in m.state_dict().items()} for m in mods]
        check(out, pm.evaluate(agents, c["actors"], sds, obs, actions, S, MIN_STD, MAX_STD), actions)
        x = torch.as_tensor(pm.stacks(obs, S)).cuda().view((T + 1) * N, S, c["n_obs"])
        for i, (o0, ow, _, _) in enumerate(agents):
            with torch.no_grad():                                        # the module's float32 forward is the kernel's up to the summation order
                assert torch.allclose(mods[i](x[:, :, o0:o0 + ow])[:, 0], torch.as_tensor(out["values"][:, :, i]).cuda().view(-1), rtol=1e-4, atol=1e-5), i
        assert not host(ppo._device()["pack"])[pad].any()                # the padding is zero and stays zero
        return out

    before = compare()
    opt = torch.optim.Adam([p for m in mods for p in m.parameters()], lr=1e-2)
    x = torch.as_tensor(pm.stacks(obs, S)).cuda().view((T + 1) * N, S, c["n_obs"])
    for i, (o0, ow, _, _) in enumerate(agents):
        mods[i](x[:, :, o0:o0 + ow]).square().sum().backward()
    opt.step()
    for i, m in enumerate(mods):
        views = ppo.parameters(i)
        assert all(p.data_ptr() == views[k].data_ptr() for k, p in m.named_parameters())          # the step was in place
    after = compare()
    assert not np.any(after["values"] == before["values"])
    assert same(after["mu"], before["mu"]) and same(after["old_log_probs"], before["old_log_probs"])     # the actors were not stepped


# ---------------------------------------------------------------------------------------------------- capture
def test_a_captured_launch_replays_the_eager_result():
    torch = pytest.importorskip("torch")
    name, S, T, N = "mixed", 5, 7, 5
    c = setup(name, S)
    ppo = make(name, S)
    obs, actions = torch.as_tensor(c["obs"][:T + 1, :N].copy()).cuda(), torch.as_tensor(c["actions"][:T, :N].copy()).cuda()
    eager = {k: host(v).copy() for k, v in ppo.evaluate(obs, actions, want_mu_std=True).items()}       # (allocates the outputs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                               # one stream, one launch: a single chain
        out = ppo.evaluate(obs, actions, want_mu_std=True)
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert same(host(v), eager[k]), k
    obs[1:].mul_(0.5)                                                    # the replay reads the tensors as they are now
    g.replay()
    torch.cuda.synchronize()
    now = {k: host(v) for k, v in out.items()}
    check(now, pm.evaluate(c["agents"], c["actors"], c["values"], host(obs), host(actions), S, MIN_STD, MAX_STD), host(actions))
    assert not same(now["values"], eager["values"])


# ---------------------------------------------------------------------------------------------------- with an env's store
def test_an_envs_store_gets_values_td_targets_and_advantages():
    torch = pytest.importorskip("torch")
    S, rows, gamma, lmbda = 4, 6, 0.99, 0.95
    env = nine(4)
    buf = env.replay_store(rows + 2, stack_size=S, seed=1)
    actors, actor_sds = env_actors(env, "ppo", S)
    store = env.rollout_store(capacity=rows)
    ppo = env.ppo_targets(actors)
    rng = np.random.default_rng(12)
    value_sds = {}
    for aid in env.possible_agents:
        o = env.obs_slices[aid]
        value_sds[aid] = random_value(rng, o.stop - o.start, S, scale=1.0)
        ppo.load_state_dict(aid, value_sds[aid])
    with pytest.raises(ValueError, match="finish\\(\\) before evaluate_store"):
        ppo.evaluate_store(store)
    roll = env.capture(lambda obs: actors.act(buf.stacked_obs()),
                       on_step=lambda obs, rew: (buf.push(actors.actions), store.record(actors.outputs["raw"].double(), None)))
    env.reset()
    buf.begin()
    store.begin()
    acted = []
    for _ in range(rows):
        roll.step()
        torch.cuda.synchronize()
        acted.append({k: host(v).copy() for k, v in actors.outputs.items()})
    assert roll.replays == rows - 1
    assert store.finish() == rows and not store.overflow
    res = ppo.evaluate_store(store, want_mu_std=True)
    adv, td_target = store.compute_gae(gamma, lmbda, normalize=True)
    torch.cuda.synchronize()
    v = {k: host(t) for k, t in store.views().items()}
    assert res["values"].data_ptr() == store.views()["values"].data_ptr()                # written straight into the store's array
    agents = ppo.agents
    raw = np.stack([a["raw"] for a in acted])
    assert same(v["actions"], raw.astype(np.float64))
    want = pm.evaluate(agents, [actor_sds[a] for a in env.possible_agents], [value_sds[a] for a in env.possible_agents], v["obs"], v["actions"], S,
                       actors.min_std, actors.max_std)
    check({k: host(t) for k, t in res.items()}, want, v["actions"])
    assert same(v["values"], want["values"])
    for t in range(rows):                                                # the distribution that is evaluated is the one that acted
        assert same(host(res["mu"])[t], acted[t]["mu"]) and same(host(res["std"])[t], acted[t]["std"]), t
    td, raw_adv = rm.td_and_gae(v["rewards"], v["values"], v["done"][:, :, None] * np.ones((1, 1, len(agents)), dtype=F), gamma, lmbda)
    assert same(v["td_target"], td) and same(host(td_target), td)
    assert same(v["advantages_raw"], raw_adv) and same(host(adv), rm.normalize_advantages(raw_adv))
    assert not v["done"].any() and np.all(v["values"][rows] != 0)       # a prefix of an episode: the bootstrap value counts
    assert same(host(ppo.evaluate_store(store)), host(res["old_log_probs"]))
    env.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    torch = pytest.importorskip("torch")
    from pednstream_amd.ppo import make_value_module

    name, S, T, N = "one", 4, 2, 3
    c = setup(name, S)
    ppo = make(name, S, load=False)
    obs, act = torch.as_tensor(c["obs"][:T + 1, :N].copy()).cuda(), torch.as_tensor(c["actions"][:T, :N].copy()).cuda()
    with pytest.raises(ValueError, match="no actor parameters"):
        ppo.evaluate(obs, act)
    ppo.actors.load_state_dict(0, c["actors"][0])
    with pytest.raises(ValueError, match="no value networks were loaded"):
        ppo.evaluate(obs, act)
    sd = dict(c["values"][0])
    with pytest.raises(ValueError, match="do not match"):
        ppo.load_state_dict(0, {k: v for k, v in sd.items() if k != "value_head.bias"})
    with pytest.raises(ValueError, match="do not match"):
        ppo.load_state_dict(0, {**sd, "ln.weight": np.zeros(64, F)})
    with pytest.raises(ValueError, match="value_head.weight: expected shape"):
        ppo.load_state_dict(0, {**sd, "value_head.weight": np.zeros((2, 64), F)})
    with pytest.raises(ValueError, match="do not match"):
        ppo.bind(0, torch.nn.Linear(2, 2).cuda())
    with pytest.raises(ValueError, match="encoder.fc1.weight: expected shape"):
        ppo.bind(0, make_value_module(5, S).cuda())
    ppo.bind(0, make_value_module(4, S).cuda())
    for bad in (obs.double(), obs.transpose(0, 1).contiguous().transpose(0, 1), obs.cpu(), obs[:, :, :3].contiguous()):
        with pytest.raises(ValueError, match="obs must"):
            ppo.evaluate(bad, act)
    for bad in (act[:1], act.half(), act.cpu(), act[:, :2], act.view(T * N, 1), host(act), torch.zeros(T, 2 * N, 1, device="cuda")[:, ::2]):
        with pytest.raises(ValueError, match="actions must"):
            ppo.evaluate(obs, bad)
    good = torch.zeros(T + 1, N, 1, device="cuda")
    for bad in (good[:T], good.double(), good.cpu(), torch.zeros(T + 1, N, 2, device="cuda")):
        with pytest.raises(ValueError, match="values_out must"):
            ppo.evaluate(obs, act, values_out=bad)
    out = ppo.evaluate(obs, act, values_out=good)
    assert out["values"] is good and good.abs().sum().item() > 0
    with pytest.raises(ValueError, match="store must be a RolloutStore"):
        ppo.evaluate_store(obs)
    env = nine(2)
    store = env.rollout_store(capacity=2, store_obs=False)
    actors, _ = env_actors(env, "ppo", S)
    with pytest.raises(ValueError, match="keeps no observations"):
        env.ppo_targets(actors).evaluate_store(store)
    with pytest.raises(ValueError, match="kind 'ppo'"):
        env.ppo_targets(env_actors(env, "sac", S)[0])
    with pytest.raises(ValueError, match="not made for this env"):
        env.ppo_targets(ppo.actors)
    env.close()
