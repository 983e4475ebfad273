"""The SAC TD targets and the Polyak update on the device (pednstream_amd/sac.py, pednstream_amd/csrc/pedn_sac.hpp) against the contract's
numpy restatement (tests/sac_target_model.py): plain tensors, drawn noise, bound torch modules, a captured update and an env's store.
The checks are staged like test_gpu_actors.check_outputs: what the contract evaluates in float32 is compared bit for bit, what it evaluates
in float64 and rounds once within 1 or 2 ulps, and every later stage is fed the kernel's own earlier outputs."""
import numpy as np
import pytest

import actor_model as am
import sac_target_model as sm
from test_gpu_actors import bits, host, nine, random_sd, same

pytestmark = pytest.mark.gpu

# (obs_w, act_w) per agent, gap before agent 1.  "mixed50": a 50-column row with act_w = 8 and a slice that starts on an odd column;
# "mixed": the actors' 67-column row with obs_w = 56 (56 columns do not fit a row of 50)
TABLES = {"one": ([(4, 1)], 0), "wide": ([(20, 4)], 0), "mixed50": ([(4, 1), (40, 8), (5, 2)], 1), "mixed": ([(4, 1), (56, 8), (6, 2)], 1)}
TILE = 8
BATCHES = (1, 3, TILE + 1, 130)       # one row, less than a tile, a tile and a row, many tiles with a ragged last one
N_MAX = 130
GAMMA, MAX_DELTA = 0.99, 2.5
F = np.float32


def within_ulps(a, b, n):
    """test_gpu_actors.within_ulps, with equal infinities counted as equal"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = (np.isnan(a) & np.isnan(b)) | (a == b)
        return bool(np.all(ok | (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= n * am.ulp(b))))


def table(name):
    widths, gap = TABLES[name]
    agents, o, a = [], 0, 0
    for i, (ow, aw) in enumerate(widths):
        o += gap if i == 1 else 0
        agents.append((o, ow, a, aw))
        o, a = o + ow, a + aw
    return agents, o, a


def random_critic(rng, obs_w, act_w, S, scale=2.0):
    from pednstream_amd.sac import critic_shapes

    sd = {}
    for key, shape in critic_shapes(obs_w, act_w, S):
        fan = shape[-1] if len(shape) == 2 else 64
        sd[key] = (rng.uniform(-1, 1, size=shape) * scale / np.sqrt(fan)).astype(np.float32)
    return sd


_setups = {}


def setup(name, S):
    """Parameters, a minibatch of N_MAX rows and noise of a case: drawn once, shared, never written."""
    key = (name, S)
    if key not in _setups:
        agents, n_obs, n_actions = table(name)
        rng = np.random.default_rng(2000 * len(name) + 10 * S)
        actors = [random_sd(rng, "sac", ow, aw, S) for (_, ow, _, aw) in agents]
        critics = [{w: random_critic(rng, ow, aw, S) for w in ("critic_1", "critic_2", "target_critic_1", "target_critic_2")} for (_, ow, _, aw) in agents]
        ns = (rng.standard_normal((N_MAX, S, n_obs)) * 2 + 1).astype(np.float32)
        rewards = rng.standard_normal((N_MAX, len(agents))).astype(np.float32)
        dones = (rng.integers(0, 4, size=N_MAX) == 0).astype(np.float32)
        noise = rng.standard_normal((N_MAX, n_actions)).astype(np.float32)
        log_alpha = rng.uniform(-3, 0.5, size=len(agents)).astype(np.float32)
        _setups[key] = dict(agents=agents, n_obs=n_obs, n_actions=n_actions, actors=actors, critics=critics, ns=ns, rewards=rewards, dones=dones,
                            noise=noise, log_alpha=log_alpha)
    return _setups[key]


_models = {}


def model_actor(name, S):
    """mu, std [N_MAX, n_actions] of the model, once per case"""
    key = (name, S)
    if key not in _models:
        c = setup(name, S)
        mu, std = np.zeros((N_MAX, c["n_actions"]), dtype=F), np.zeros((N_MAX, c["n_actions"]), dtype=F)
        for (o0, ow, a0, aw), sd in zip(c["agents"], c["actors"]):
            mu[:, a0:a0 + aw], _, std[:, a0:a0 + aw] = am.forward("sac", sd, c["ns"][:, :, o0:o0 + ow])
        _models[key] = (mu, std)
    return _models[key]


def make(name, S, tau=0.005, seed=0, load=True, **kw):
    torch = pytest.importorskip("torch")
    from pednstream_amd.policy import StackedActors
    from pednstream_amd.sac import SacTargets

    c = setup(name, S)
    low, high = np.zeros(c["n_actions"], dtype=F), np.full(c["n_actions"], 4.0, dtype=F)
    actors = StackedActors("sac", c["agents"], low, high, 1, c["n_obs"], c["n_actions"], stack_size=S, delta_actions=False, max_delta=MAX_DELTA)
    sac = SacTargets(actors, gamma=GAMMA, tau=tau, seed=seed, **kw)
    if load:
        for i in range(len(c["agents"])):
            actors.load_state_dict(i, c["actors"][i])
            for which, sd in c["critics"][i].items():
                sac.load_state_dict(i, which, sd)
        sac.log_alpha.copy_(torch.as_tensor(c["log_alpha"]))
    return sac


def run(torch, sac, c, rows, noise=True, ns=None, rewards=None, noise_values=None):
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()
    ns = c["ns"][rows] if ns is None else ns
    rewards = c["rewards"][rows] if rewards is None else rewards
    nz = (c["noise"][rows] if noise_values is None else noise_values) if noise else None
    td = sac.td_target(dev(rewards), dev(ns), dev(c["dones"][rows]), noise=dev(nz) if noise else None)
    out = {k: host(v) for k, v in sac.outputs.items()}
    assert td.data_ptr() == sac.outputs["td_target"].data_ptr() and same(host(td), out["td_target"])
    return out


def check(agents, actors, targets, log_alpha, ns, rewards, dones, out, want_mu=None, want_std=None, want_eps=None):
    """The staged comparison of one launch's outputs with the model.  targets[i] = (target_critic_1, target_critic_2) state dicts."""
    B = ns.shape[0]
    assert out["mu"].shape == (B, out["mu"].shape[1]) and out["td_target"].shape == (B, len(agents))
    if want_mu is not None:
        assert same(out["mu"], want_mu), "mu"
        assert within_ulps(out["std"], want_std, 1), "std"
    if want_eps is not None:
        assert same(out["eps"], want_eps), "eps"
    for i, ((o0, ow, a0, aw), (t1, t2)) in enumerate(zip(agents, targets)):
        sl, x = slice(a0, a0 + aw), ns[:, :, o0:o0 + ow]
        if want_mu is None:                                              # (the caller has no shared model forward: evaluate it here)
            mu, _, std = am.forward("sac", actors[i], x)
            assert same(out["mu"][:, sl], mu), ("mu", i)
            assert within_ulps(out["std"][:, sl], std, 1), ("std", i)
        u, t, na, logp = sm.tail(out["mu"][:, sl], out["std"][:, sl], out["eps"][:, sl], MAX_DELTA)
        assert within_ulps(out["next_actions"][:, sl], na, 2), ("next_actions", i)
        assert within_ulps(out["logp"][:, sl], logp, 2), ("logp", i)
        assert same(out["entropy"][:, i], sm.entropy(out["logp"][:, sl])), ("entropy", i)
        assert same(out["q1"][:, i], sm.critic(t1, x, out["next_actions"][:, sl])), ("q1", i)
        assert same(out["q2"][:, i], sm.critic(t2, x, out["next_actions"][:, sl])), ("q2", i)
        want = sm.td(out["q1"][:, i], out["q2"][:, i], out["entropy"][:, i], log_alpha[i], rewards[:, i], dones, GAMMA)
        assert same(out["td_target"][:, i], want), ("td_target", i)


def targets_of(c):
    return [(cr["target_critic_1"], cr["target_critic_2"]) for cr in c["critics"]]


# ---------------------------------------------------------------------------------------------------- plain tensors
@pytest.mark.parametrize("S", [1, 4, 5])
@pytest.mark.parametrize("name", list(TABLES))
def test_kernel_equals_the_model(name, S):
    torch = pytest.importorskip("torch")
    c = setup(name, S)
    mu, std = model_actor(name, S)
    sac = make(name, S)
    whole = None
    for B in BATCHES:
        rows = slice(0, B)
        out = run(torch, sac, c, rows)
        check(c["agents"], c["actors"], targets_of(c), c["log_alpha"], c["ns"][rows], c["rewards"][rows], c["dones"][rows], out, mu[rows], std[rows],
              c["noise"][rows])
        whole = out if B == N_MAX else whole
    assert sac.draws() == 0                                              # supplied noise is no draw
    lower = whole["q2"] < whole["q1"]
    assert lower.any() and not lower.all()                               # the minimum switches between the critics
    # row independence: row 77 of the 130-row launch alone, as row 0 of a launch of one
    out = run(torch, sac, c, slice(77, 78))
    for k, v in out.items():
        assert same(v, whole[k][77:78]), k
    first = sac.td_target(*[torch.as_tensor(c[k][:3]).cuda() for k in ("rewards", "ns", "dones")], noise=torch.as_tensor(c["noise"][:3]).cuda())
    again = sac.td_target(*[torch.as_tensor(c[k][:3]).cuda() for k in ("rewards", "ns", "dones")], noise=torch.as_tensor(c["noise"][:3]).cuda())
    assert first.data_ptr() == again.data_ptr()                          # allocated once per batch size


def test_the_acting_kernel_computes_the_same_mu_std_and_eps():
    """sac_target_kernel's actor wave against actor_forward_kernel (kind "sac") on the same weights, stacks and noise, bit for bit.  The
    smallest shapes that reach every branch of the shared layer: 9 rows are a full SAC tile of 8 and a ragged one, and for the actors
    one workgroup with 23 dead envs; K1 = 5 * 7 = 35 is a full chunk and a tail of 3, which takes the scalar remainder loop; the heads
    are layers of 2 and of 16 rows."""
    torch = pytest.importorskip("torch")
    from pednstream_amd.policy import StackedActors
    from pednstream_amd.sac import SacTargets

    B, S, agents, n_obs, n_actions = TILE + 1, 5, [(0, 7, 0, 1), (7, 7, 1, 8)], 14, 9
    rng = np.random.default_rng(35)
    low, high = np.zeros(n_actions, dtype=F), np.full(n_actions, 4.0, dtype=F)
    actors = StackedActors("sac", agents, low, high, B, n_obs, n_actions, stack_size=S, delta_actions=False, max_delta=MAX_DELTA)
    sac = SacTargets(actors, gamma=GAMMA)
    for i, (_, ow, _, aw) in enumerate(agents):
        actors.load_state_dict(i, random_sd(rng, "sac", ow, aw, S))
        for which in ("target_critic_1", "target_critic_2"):
            sac.load_state_dict(i, which, random_critic(rng, ow, aw, S))
    dev = lambda v: torch.as_tensor(v).cuda()
    stack = dev((rng.standard_normal((B, S, n_obs)) * 2 + 1).astype(F))
    noise = rng.standard_normal((B, n_actions)).astype(F)
    actors.act(stack, noise=dev(noise))
    acted = {k: host(v) for k, v in actors.outputs.items()}
    sac.td_target(dev(rng.standard_normal((B, len(agents))).astype(F)), stack, dev(np.zeros(B, dtype=F)), noise=dev(noise))
    out = {k: host(v) for k, v in sac.outputs.items()}
    assert same(acted["eps"], noise) and np.all(acted["std"] > 0) and np.all(acted["mu"] != 0)          # (the launches wrote every column)
    for k in ("mu", "std", "eps"):
        assert same(out[k], acted[k]), k


def test_awkward_values_stay_in_their_row():
    torch = pytest.importorskip("torch")
    name, S, B = "mixed", 4, 20
    c = setup(name, S)
    rows = slice(0, B)
    sac = make(name, S)
    clean = run(torch, sac, c, rows)
    ns, rewards, noise = c["ns"][rows].copy(), c["rewards"][rows].copy(), c["noise"][rows].copy()
    ns[3, 1, :] = np.nan                                                 # a NaN frame
    ns[5, :, ::3] = -0.0
    ns[6, :, ::2] = 0.0
    ns[9, 2, 7] = np.inf                                                 # one column of agent 1, in the second tile
    ns[10, 0, 2] = -np.inf                                               # agent 0
    rewards[12, 1] = np.nan
    rewards[13, 2] = -np.inf
    noise[15, 0] = np.inf
    noise[16, 3] = np.nan
    touched = (3, 5, 6, 9, 10, 12, 13, 15, 16)
    out = run(torch, sac, c, rows, ns=ns, rewards=rewards, noise_values=noise)
    check(c["agents"], c["actors"], targets_of(c), c["log_alpha"], ns, rewards, c["dones"][rows], out, want_eps=noise)
    for k, v in out.items():
        for b in range(B):
            if b not in touched:
                assert same(v[b], clean[k][b]), (k, b)
    assert np.isnan(out["td_target"][3]).all() and np.isnan(out["mu"][3]).all()
    assert np.isnan(out["td_target"][9, 1]) and np.isfinite(out["td_target"][9, [0, 2]]).all()
    assert np.isnan(out["td_target"][10, 0]) and np.isfinite(out["td_target"][10, 1:]).all()
    assert np.isnan(out["td_target"][12, 1]) and out["td_target"][13, 2] == -np.inf
    assert not np.isfinite(out["td_target"][15, 0]) and np.isfinite(out["td_target"][15, 1:]).all()
    assert np.isnan(out["td_target"][16, 1]) and np.isfinite(out["td_target"][16, [0, 2]]).all()
    assert np.isfinite(out["td_target"][[5, 6]]).all()


# ---------------------------------------------------------------------------------------------------- drawn noise
def test_drawn_noise_is_the_contracts():
    torch = pytest.importorskip("torch")
    name, S, B = "mixed", 4, 130
    c = setup(name, S)
    mu, std = model_actor(name, S)
    seed = 0x5EED_0000_0000_0073
    sac = make(name, S, seed=seed)
    b, col = np.arange(B)[:, None], np.arange(c["n_actions"])[None, :]
    rows = slice(0, B)
    runs = []
    for d in (0, 1):
        out = run(torch, sac, c, rows, noise=False)
        want = sm.noise(seed, b, col, d)
        tol = 2.0 ** -23 * np.maximum(np.abs(want.astype(np.float64)), 2.0 ** -10)
        assert np.all(np.abs(out["eps"].astype(np.float64) - want) <= tol), d
        check(c["agents"], c["actors"], targets_of(c), c["log_alpha"], c["ns"], c["rewards"], c["dones"], out, mu, std)
        runs.append(out["eps"])
        assert sac.draws() == d + 1
    assert not same(runs[0], runs[1])
    run(torch, sac, c, rows)                                             # given noise: no draw
    assert sac.draws() == 2
    again = make(name, S, seed=seed)
    assert same(run(torch, again, c, rows, noise=False)["eps"], runs[0])
    # a row's draw depends on its position and the counter alone: the first 9 rows of a smaller launch
    assert same(run(torch, make(name, S, seed=seed), c, slice(0, 9), noise=False)["eps"], runs[0][:9])
    other = make(name, S, seed=seed + 1)
    assert not np.any(bits(run(torch, other, c, rows, noise=False)["eps"]) == bits(runs[0]))
    # not the actors' stream
    assert not np.any(bits(am.noise(seed, b, col, 0)) == bits(runs[0]))


# ---------------------------------------------------------------------------------------------------- the Polyak update
@pytest.mark.parametrize("tau", [0.0, 0.005, 1.0])
def test_soft_update_is_torchs(tau):
    torch = pytest.importorskip("torch")
    name, S = "mixed", 5
    c = setup(name, S)
    sac = make(name, S, tau=tau)
    d = sac._device()
    online, target = d["online"].clone(), d["target"].clone()
    pad = np.ones(sac.pack_size, dtype=bool)
    for pair in sac.offsets:
        for cur in pair:
            for at, shape in cur.values():
                pad[at:at + int(np.prod(shape))] = False
    assert pad.any() and sac.pack_size % 4 == 0 and all(at % 4 == 0 for at in sac.critic_table.reshape(-1))
    assert not host(online)[pad].any() and not host(target)[pad].any()
    for n in (1, 2):
        sac.soft_update()
        want = target * (1.0 - tau) + online * tau                       # the reference's line, on the device
        got = d["target"]
        assert same(host(got), host(want)), n
        assert same(host(got), sm.polyak(host(target), host(online), tau)), n
        assert same(host(d["online"]), host(online))
        assert not host(got)[pad].any()
        target = got.clone()
    if tau == 0.0:
        assert same(host(target), host(d["target"])) and not same(host(target), host(online))
    if tau == 1.0:
        assert same(host(target), host(online))
    # what the launch wrote is what the next td_target reads
    rows = slice(0, 9)
    out = run(torch, sac, c, rows)
    t = host(d["target"])
    now = [tuple({k: t[at:at + int(np.prod(shape))].reshape(shape) for k, (at, shape) in cur.items()} for cur in pair) for pair in sac.offsets]
    check(c["agents"], c["actors"], now, c["log_alpha"], c["ns"][rows], c["rewards"][rows], c["dones"][rows], out)


# ---------------------------------------------------------------------------------------------------- bound modules
def test_bind_makes_the_optimiser_update_what_the_kernels_read():
    torch = pytest.importorskip("torch")
    from pednstream_amd.sac import WHICH, make_critic_module

    name, S, B = "mixed", 4, 40
    c = setup(name, S)
    agents = c["agents"]
    sac = make(name, S, tau=0.25)
    torch.manual_seed(2)
    ns, rewards, dones, noise = (torch.as_tensor(c[k][:B]).cuda() for k in ("ns", "rewards", "dones", "noise"))
    mods, alphas = [], []
    for i, (o0, ow, a0, aw) in enumerate(agents):
        four = [make_critic_module(ow, aw, S).cuda() for _ in WHICH]
        la = torch.tensor(-1.0 - i, device="cuda", requires_grad=True)
        sac.bind(i, *four, log_alpha=la)
        for which, m in zip(WHICH, four):
            views = sac.parameters(i, which)
            assert all(p.data_ptr() == views[k].data_ptr() for k, p in m.named_parameters())
        assert la.data_ptr() == sac.log_alpha[i:i + 1].data_ptr() and sac.log_alpha[i].item() == -1.0 - i
        mods.append(four)
        alphas.append(la)

    def compare():
        sac.td_target(rewards, ns, dones, noise=noise)
        out = sac.outputs
        for i, (o0, ow, a0, aw) in enumerate(agents):
            x, na = ns[:, :, o0:o0 + ow], out["next_actions"][:, a0:a0 + aw]
            with torch.no_grad():
                q1, q2 = mods[i][2](x, na)[:, 0], mods[i][3](x, na)[:, 0]
                # the module's float32 forward is the kernel's up to the summation order
                assert torch.allclose(q1, out["q1"][:, i], rtol=1e-4, atol=1e-5), i
                assert torch.allclose(q2, out["q2"][:, i], rtol=1e-4, atol=1e-5), i
                ent = -out["logp"][:, a0:a0 + aw].sum(dim=1)
                td = rewards[:, i] + GAMMA * (torch.min(q1, q2) + alphas[i].exp() * ent) * (1 - dones)
                assert torch.allclose(td, out["td_target"][:, i], rtol=1e-4, atol=1e-5), i
        return {k: host(v) for k, v in out.items()}

    before = compare()
    # one optimiser step on every critic (the targets' gradients stay None: Adam skips them) and on log_alpha
    opt = torch.optim.Adam([p for four in mods for m in four[:2] for p in m.parameters()] + alphas, lr=1e-2)
    for i, (o0, ow, a0, aw) in enumerate(agents):
        x, a = ns[:, :, o0:o0 + ow], noise[:, a0:a0 + aw]
        (mods[i][0](x, a).square().sum() + mods[i][1](x, a).sum() + alphas[i] * 3).backward()
    t_before = host(sac._device()["target"]).copy()
    opt.step()
    for i in range(len(agents)):
        for which, m in zip(WHICH, mods[i]):
            views = sac.parameters(i, which)
            assert all(p.data_ptr() == views[k].data_ptr() for k, p in m.named_parameters())      # the step was in place
    after_step = compare()                                               # log_alpha moved: td moves, q does not (the targets are untouched)
    assert same(after_step["q1"], before["q1"]) and not same(after_step["td_target"], before["td_target"])
    assert same(host(sac._device()["target"]), t_before)
    sac.soft_update()                                                    # reads the stepped online critics, writes the target modules
    assert same(host(sac._device()["target"]), sm.polyak(t_before, host(sac._device()["online"]), 0.25))
    after_update = compare()
    assert not same(after_update["q1"], before["q1"]) and not same(after_update["q2"], before["q2"])
    # and against the model, from the modules' state dicts
    now = [tuple({k: host(v) for k, v in m.state_dict().items()} for m in four[2:]) for four in mods]
    la = np.array([a.item() for a in alphas], dtype=F)
    check(agents, c["actors"], now, la, c["ns"][:B], c["rewards"][:B], c["dones"][:B], after_update, want_eps=c["noise"][:B])


# ---------------------------------------------------------------------------------------------------- with an env
def env_update(torch, how, S=4, B=16, iterations=3):
    """An env's store filled by its actors, then sample -> td_target -> soft_update: one warm iteration (it allocates), then `iterations`
    recorded ones, eager or as replays of ONE captured graph."""
    from test_gpu_actors import env_actors

    env = nine(8)
    buf = env.replay_store(3, stack_size=S, seed=1)
    actors, actor_sds = env_actors(env, "sac", S)
    sac = env.sac_targets(actors, tau=0.1, seed=5)
    rng = np.random.default_rng(9)
    critics = {}
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        critics[aid] = {w: random_critic(rng, o.stop - o.start, a.stop - a.start, S, scale=1.0) for w in ("critic_1", "critic_2", "target_critic_1", "target_critic_2")}
        for w, sd in critics[aid].items():
            sac.load_state_dict(aid, w, sd)
    env.reset()
    buf.begin()
    for _ in range(5):
        a = actors.act(buf.stacked_obs())
        env.step_device(a, sync=True)
        buf.push(a)

    def update():
        s, a, r, ns, d, idx = buf.sample(B)
        sac.td_target(r, ns, d)
        sac.soft_update()
        return r, ns, d

    keep = lambda r, ns, d: ({k: host(v) for k, v in sac.outputs.items()}, host(r), host(ns), host(d), host(sac._device()["target"]))
    log = []
    first = keep(*update())
    torch.cuda.synchronize()
    if how == "graph":
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):                           # one stream: three launches in a row
            r, ns, d = update()
        for _ in range(iterations):
            g.replay()
            torch.cuda.synchronize()
            log.append(keep(r, ns, d))
    else:
        for _ in range(iterations):
            out = update()
            torch.cuda.synchronize()
            log.append(keep(*out))
    assert sac.draws() == iterations + 1 and buf.state()["draws"] == iterations + 1
    info = dict(agents=sac.agents, actors=[actor_sds[aid] for aid in env.possible_agents], critics=[critics[aid] for aid in env.possible_agents],
                log_alpha=host(sac.log_alpha), seed=5, n_actions=env.n_actions)
    env.close()
    return first, log, info


def test_an_envs_minibatch_and_a_captured_update():
    torch = pytest.importorskip("torch")
    first, eager, info = env_update(torch, "eager")
    # the env's own table: the first update against the model, with the noise of draw 0
    out, r, ns, d, _ = first
    assert r.shape == (16, len(info["agents"])) and ns.shape[0] == 16 and np.isfinite(out["td_target"]).all()
    want = sm.noise(info["seed"], np.arange(16)[:, None], np.arange(info["n_actions"])[None, :], 0)
    assert np.all(np.abs(out["eps"].astype(np.float64) - want) <= 2.0 ** -23 * np.maximum(np.abs(want.astype(np.float64)), 2.0 ** -10))
    targets = [(cr["target_critic_1"], cr["target_critic_2"]) for cr in info["critics"]]
    check(info["agents"], info["actors"], targets, info["log_alpha"], ns, r, d, out)
    _, graph, _ = env_update(torch, "graph")
    assert len(eager) == len(graph) == 3
    for t, (a, b) in enumerate(zip(eager, graph)):
        for k in a[0]:
            assert same(a[0][k], b[0][k]), (t, k)
        for x, y, what in zip(a[1:], b[1:], ("rewards", "next_states", "dones", "target pack")):
            assert same(x, y), (t, what)
    assert not same(eager[0][0]["eps"], eager[1][0]["eps"]) and not same(eager[0][4], eager[2][4])      # every replay draws and updates anew


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    torch = pytest.importorskip("torch")
    from pednstream_amd.policy import StackedActors
    from pednstream_amd.rl_env import MultiScenarioVecEnv
    from pednstream_amd.sac import SacTargets, make_critic_module

    name, S, B = "one", 4, 3
    c = setup(name, S)
    low, high = np.zeros(1, dtype=F), np.ones(1, dtype=F)
    ppo = StackedActors("ppo", c["agents"], low, high, 1, c["n_obs"], c["n_actions"], stack_size=S)
    with pytest.raises(ValueError, match="kind 'sac'"):
        SacTargets(ppo)
    with pytest.raises(ValueError, match="StackedActors"):
        SacTargets(None)
    actors = StackedActors("sac", c["agents"], low, high, 1, c["n_obs"], c["n_actions"], stack_size=S)
    for tau in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="tau"):
            SacTargets(actors, tau=tau)
    for gamma in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            SacTargets(actors, gamma=gamma)
    assert hasattr(MultiScenarioVecEnv, "sac_targets")
    with pytest.raises(ValueError, match="separate engines"):
        MultiScenarioVecEnv.sac_targets(None, actors)

    sac = SacTargets(actors)
    r, ns, d, nz = (torch.as_tensor(c[k][:B]).cuda() for k in ("rewards", "ns", "dones", "noise"))
    with pytest.raises(ValueError, match="no actor parameters"):
        sac.td_target(r, ns, d)
    actors.load_state_dict(0, c["actors"][0])
    with pytest.raises(ValueError, match="no critics were loaded"):
        sac.td_target(r, ns, d)
    with pytest.raises(ValueError, match="no critics were loaded"):
        sac.soft_update()
    with pytest.raises(ValueError, match="td_target\\(\\) has not run"):
        sac.outputs
    with pytest.raises(ValueError, match="Unknown agent"):
        sac.load_state_dict(5, "critic_1", c["critics"][0]["critic_1"])
    with pytest.raises(ValueError, match="which must be"):
        sac.load_state_dict(0, "critic_3", c["critics"][0]["critic_1"])
    with pytest.raises(ValueError, match="which must be"):
        sac.parameters(0, "actor")
    sd = dict(c["critics"][0]["critic_1"])
    with pytest.raises(ValueError, match="do not match"):
        sac.load_state_dict(0, "critic_1", {k: v for k, v in sd.items() if k != "fc_out.bias"})
    with pytest.raises(ValueError, match="do not match"):
        sac.load_state_dict(0, "critic_1", {**sd, "ln.weight": np.zeros(64, F)})
    with pytest.raises(ValueError, match="fc.weight: expected shape"):
        sac.load_state_dict(0, "critic_1", {**sd, "fc.weight": np.zeros((64, 64), F)})
    with pytest.raises(ValueError, match="do not match"):
        sac.bind(0, *[torch.nn.Linear(2, 2).cuda() for _ in range(4)])
    four = [make_critic_module(4, 1, S).cuda() for _ in range(4)]
    with pytest.raises(ValueError, match="log_alpha must be"):
        sac.bind(0, *four, log_alpha=torch.zeros(2, device="cuda"))
    for which, sd in c["critics"][0].items():
        sac.load_state_dict(0, which, sd)
    for bad in (ns[:2], ns.double(), ns.transpose(1, 2), ns.view(B, S * c["n_obs"]), ns.cpu(), host(ns)):
        with pytest.raises(ValueError, match="next_states must"):
            sac.td_target(r, bad, d)
    for bad in (r[:2], r.double(), r.view(-1), r.cpu()):
        with pytest.raises(ValueError, match="rewards must"):
            sac.td_target(bad, ns, d)
    for bad in (d.view(B, 1), d.double(), d.cpu(), torch.zeros(0, device="cuda"), torch.zeros(2 * B, device="cuda")[::2]):
        with pytest.raises(ValueError, match="dones must"):
            sac.td_target(r, ns, bad)
    for bad in (nz[:2], nz.double(), nz.cpu(), torch.zeros(B, 2, device="cuda")):
        with pytest.raises(ValueError, match="noise must"):
            sac.td_target(r, ns, d, noise=bad)
    sac.td_target(r, ns, d, noise=nz)
    sac.soft_update()
    assert sac.draws() == 0
