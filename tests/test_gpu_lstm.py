"""The LSTM PPO agents on the device (pednstream_amd/lstm.py, pednstream_amd/csrc/pedn_lstm.hpp) against the contract's numpy restatement
(tests/lstm_model.py): the acting launch step by step, the sequence launch, the recurrent state, drawn noise, bound torch modules, the GAE
with next values of their own, and an env's captured rollout.  What the contract evaluates in float32 (h, c, mu, values) is compared bit
for bit, std within 1 ulp (its softplus is a float64 evaluation rounded once: the pre-softplus value is no output of a launch, std is
where it shows), raw within 2 ulps of the model's tail fed the kernel's own mu, std and eps, and the log-probability within 2 ulps of
the model's fed the kernel's own mu and std: the allowances of tests/test_gpu_actors.py and tests/test_gpu_ppo_eval.py."""
import numpy as np
import pytest

import actor_model as am
import lstm_model as lm
import ppo_eval_model as pm
import rollout_model as rm
from golden_util import DATA
from test_gpu_actors import bits, host, same, within_ulps

pytestmark = pytest.mark.gpu

F = np.float32
# (obs0, obs_w, act0, act_w): obs_w 1, 33 (one more than a chunk of 32 inputs) and 20; act_w 8 is the most an agent has.  Observation
# columns 0-1, 3-5, 39-40 and 61-64 and action columns 1 and 10 belong to nobody.
AGENTS = [(2, 1, 0, 1), (6, 33, 2, 8), (41, 20, 11, 3)]
N_OBS, N_ACTIONS = 65, 14
OWNED = np.zeros(N_ACTIONS, dtype=bool)
for _, _, _a0, _aw in AGENTS:
    OWNED[_a0:_a0 + _aw] = True
N_ENVS = (1, 33, 70)                  # 33, 70: a partial second and third tile of 32 envs
T_MAX, N_MAX = 9, 70
T_SEQ = (1, 2, 9)
SENTINEL = -77.25
MIN_STD, MAX_STD = 1e-3, 10.0


def random_sd(rng, shapes, scale=2.0):
    sd = {}
    for key, shape in shapes:
        fan = shape[-1] if len(shape) == 2 else 64
        sd[key] = (rng.uniform(-1, 1, size=shape) * scale / np.sqrt(fan)).astype(F)
    return sd


_setup = {}


def setup():
    """Parameters, the observations, actions and noise of a (T_MAX, N_MAX) rollout and the model's outputs for it: made once, shared,
    never written.  A row's numbers depend on its own env's frames up to its time only, so the model of a smaller (T, N) is the corner
    [:T, :N] of this one."""
    if not _setup:
        from pednstream_amd.lstm import actor_tensor_shapes, value_tensor_shapes

        rng = np.random.default_rng(1704)
        c = _setup
        c["actors"] = [random_sd(rng, actor_tensor_shapes(ow, aw)) for (_, ow, _, aw) in AGENTS]
        c["values"] = [random_sd(rng, value_tensor_shapes(ow)) for (_, ow, _, _) in AGENTS]
        c["obs"] = (rng.standard_normal((T_MAX + 1, N_MAX, N_OBS)) * 2 + 1).astype(F)
        c["actions"] = (rng.standard_normal((T_MAX, N_MAX, N_ACTIONS)) * 1.5).astype(F)
        c["noise"] = rng.standard_normal((T_MAX, N_MAX, N_ACTIONS)).astype(F)
        c["low"], c["high"] = np.full(N_ACTIONS, -1.0, dtype=F), rng.uniform(2, 6, size=N_ACTIONS).astype(F)
        c["model"] = lm.evaluate(AGENTS, c["actors"], c["values"], c["obs"], c["actions"], MIN_STD, MAX_STD)
    return _setup


def make(n_envs, load=True, delta=False, agents=AGENTS, **kw):
    pytest.importorskip("torch")
    from pednstream_amd.lstm import LstmActors, LstmPpoTargets

    c = setup()
    actors = LstmActors(agents, c["low"], c["high"], n_envs, N_OBS, N_ACTIONS, delta_actions=delta, min_std=MIN_STD, max_std=MAX_STD, **kw)
    ppo = LstmPpoTargets(actors)
    if load:
        for i in range(len(agents)):
            actors.load_state_dict(i, c["actors"][i])
            ppo.load_state_dict(i, c["values"][i])
    return actors, ppo


def dev(torch, v):
    return torch.as_tensor(np.ascontiguousarray(v)).cuda()


def model_tail(mu, std, eps, obs_rows, delta, deterministic=False, agents=AGENTS, max_delta=2.5):
    """raw, actions of the model from the given mu / std / eps rows (the columns some agent owns)."""
    c = setup()
    raw, act = np.zeros(mu.shape, dtype=F), np.zeros(mu.shape, dtype=np.float64)
    for (o0, ow, a0, aw) in agents:
        sl = slice(a0, a0 + aw)
        width = lm.widths(obs_rows[:, o0:o0 + ow], aw) if delta else np.zeros((mu.shape[0], aw), dtype=F)
        raw[:, sl], _ = am.act_tail("ppo", mu[:, sl], std[:, sl], eps[:, sl], width, c["low"][sl], c["high"][sl], delta_actions=delta,
                                    max_delta=max_delta, deterministic=deterministic)
        act[:, sl] = am.actions_of(raw[:, sl], width, c["low"][sl], c["high"][sl], delta)
    return raw, act


def act_steps(torch, actors, obs, noise=None, steps=None, fill=True):
    """`steps` consecutive launches on obs[t]; per step the outputs, the actions and the state behind it (host copies)."""
    log = []
    for t in range(obs.shape[0] - 1 if steps is None else steps):
        if fill:                                                         # columns nobody owns must come back untouched
            for v in actors.outputs.values():
                v.fill_(SENTINEL)
            actors.actions.fill_(SENTINEL)
        act = actors.act(dev(torch, obs[t]), noise=None if noise is None else dev(torch, noise[t]))
        assert act is actors.actions
        log.append({**{k: host(v).copy() for k, v in actors.outputs.items()}, "actions": host(act).copy(),
                    "h": host(actors.hidden["h"]).copy(), "c": host(actors.hidden["c"]).copy()})
    return log


def check_step(got, m, t, n, obs_rows, eps_in, delta=False, deterministic=False, agents=AGENTS, max_delta=2.5):
    """One acting launch against the model m (lstm_model.evaluate's dict) at step t for envs [0, n)."""
    assert same(got["h"], m["h"][:, t, :n]) and same(got["c"], m["c"][:, t, :n]), ("state", t)
    assert same(got["mu"][:, OWNED], m["mu"][t, :n][:, OWNED]), ("mu", t)
    assert within_ulps(got["std"][:, OWNED], m["std"][t, :n][:, OWNED], 1), ("std", t)
    assert same(got["eps"][:, OWNED], eps_in[:, OWNED]), ("eps", t)
    raw, _ = model_tail(got["mu"], got["std"], got["eps"], obs_rows, delta, deterministic, agents, max_delta)
    assert within_ulps(got["raw"][:, OWNED], raw[:, OWNED], 2), ("raw", t)
    raw_in = np.where(OWNED, got["raw"], 0).astype(F)
    for (o0, ow, a0, aw) in agents:                                      # the actions are the kernel's own raw, delta and clip applied
        sl = slice(a0, a0 + aw)
        width = lm.widths(obs_rows[:, o0:o0 + ow], aw) if delta else 0
        assert same(got["actions"][:, sl], am.actions_of(raw_in[:, sl], width, setup()["low"][sl], setup()["high"][sl], delta)), ("actions", t)
    for k in ("mu", "std", "eps", "raw", "actions"):
        assert np.all(got[k][:, ~OWNED] == SENTINEL), (k, t)             # columns nobody owns come back untouched


# ---------------------------------------------------------------------------------------------------- the acting launch
@pytest.mark.parametrize("n", N_ENVS)
def test_acting_equals_the_model_step_by_step(n):
    torch = pytest.importorskip("torch")
    c = setup()
    actors, _ = make(n)
    assert not host(actors.hidden["h"]).any() and not host(actors.hidden["c"]).any()      # a fresh object starts from zeros
    log = act_steps(torch, actors, c["obs"][:, :n], c["noise"][:, :n])
    assert len(log) == T_MAX
    for t, got in enumerate(log):
        check_step(got, c["model"], t, n, c["obs"][t, :n], c["noise"][t, :n])
    assert actors.draws() == 0                                           # supplied noise is no draw
    assert not same(log[0]["h"], log[1]["h"]) and np.isfinite(log[-1]["actions"][:, OWNED]).all()


def test_delta_actions_add_the_width_of_the_single_frame():
    torch = pytest.importorskip("torch")
    from pednstream_amd.lstm import actor_tensor_shapes

    agents = [(2, 1, 0, 1), (6, 32, 2, 8), (41, 21, 11, 3)]              # act_w divides obs_w (the reference's reshape); the same action columns
    c = setup()
    n, T, max_delta = 33, 3, 0.75
    actors, _ = make(n, load=False, delta=True, agents=agents, max_delta=max_delta)
    rng = np.random.default_rng(8)
    sds = [random_sd(rng, actor_tensor_shapes(ow, aw)) for (_, ow, _, aw) in agents]
    for i, sd in enumerate(sds):
        actors.load_state_dict(i, sd)
    model = lm.evaluate(agents, sds, [None] * len(agents), c["obs"][:T + 1, :n], c["actions"][:T, :n], MIN_STD, MAX_STD)
    log = act_steps(torch, actors, c["obs"][:T + 1, :n], c["noise"][:, :n])
    for t, got in enumerate(log):
        check_step(got, model, t, n, c["obs"][t, :n], c["noise"][t, :n], delta=True, agents=agents, max_delta=max_delta)
        assert np.all(np.abs(got["raw"][:, OWNED]) <= F(max_delta)) and np.any(np.abs(got["raw"][:, OWNED]) == F(max_delta))
        assert not same(got["actions"][:, OWNED], got["raw"][:, OWNED].astype(np.float64))


def test_position_independence_of_both_launches():
    """Env 0 alone equals the same data placed at env 40 of 70."""
    torch = pytest.importorskip("torch")
    c = setup()
    e = 40
    whole_a, whole_p = make(N_MAX)
    one_a, one_p = make(1)
    whole = act_steps(torch, whole_a, c["obs"], c["noise"], fill=False)
    one = act_steps(torch, one_a, c["obs"][:, e:e + 1], c["noise"][:, e:e + 1], fill=False)
    for t in range(T_MAX):
        for k in ("mu", "std", "eps", "raw", "actions"):
            assert same(one[t][k], whole[t][k][e:e + 1]), (k, t)
        for k in ("h", "c"):
            assert same(one[t][k], whole[t][k][:, e:e + 1]), (k, t)
    w = {k: host(v) for k, v in whole_p.evaluate(dev(torch, c["obs"]), dev(torch, c["actions"]), want_mu_std=True).items()}
    o = {k: host(v) for k, v in one_p.evaluate(dev(torch, c["obs"][:, e:e + 1]), dev(torch, c["actions"][:, e:e + 1]), want_mu_std=True).items()}
    for k in w:
        assert same(o[k], w[k][:, e:e + 1]), k


def test_reset_hidden_zeroes_exactly_the_masked_envs():
    torch = pytest.importorskip("torch")
    c = setup()
    n = N_MAX
    actors, _ = make(n)
    act_steps(torch, actors, c["obs"], c["noise"], steps=2, fill=False)
    before = {k: host(v).copy() for k, v in actors.hidden.items()}
    assert all(np.all(v != 0) for v in before.values())
    mask = np.zeros(n, dtype=bool)
    mask[[0, 31, 32, 69]] = True
    actors.reset_hidden(dev(torch, mask))
    after = {k: host(v) for k, v in actors.hidden.items()}
    for k in after:
        assert not after[k][:, mask].any() and not np.signbit(after[k][:, mask]).any(), k
        assert same(after[k][:, ~mask], before[k][:, ~mask]), k
    # the masked envs start over: their next step is the model's first step on that observation
    got = act_steps(torch, actors, c["obs"][:1], c["noise"][:1], steps=1, fill=False)[0]
    m = c["model"]
    assert same(got["h"][:, mask], m["h"][:, 0][:, mask]) and same(got["mu"][mask][:, OWNED], m["mu"][0][mask][:, OWNED])
    assert not same(got["h"][:, ~mask], m["h"][:, 0][:, ~mask])
    actors.reset_hidden(dev(torch, mask.astype(np.uint8)))                 # uint8 is read the same way
    assert not host(actors.hidden["h"])[:, mask].any()
    actors.reset_hidden()
    assert not host(actors.hidden["h"]).any() and not host(actors.hidden["c"]).any()


def test_noise_drawn_given_and_none():
    torch = pytest.importorskip("torch")
    c = setup()
    n, seed = N_MAX, 0x5EED_0000_0000_0074
    obs = dev(torch, c["obs"][0])
    g, col = np.arange(n)[:, None], np.arange(N_ACTIONS)[None, :]
    actors, _ = make(n, seed=seed)
    runs = []
    for d in (0, 1):
        actors.act(obs)
        want = lm.noise(seed, g, col, d)
        eps = host(actors.outputs["eps"]).copy()
        tol = 2.0 ** -23 * np.maximum(np.abs(want.astype(np.float64)), 2.0 ** -10)
        assert np.all(np.abs(eps.astype(np.float64) - want)[:, OWNED] <= tol[:, OWNED]), d
        runs.append(eps)
    assert actors.draws() == 2 and not same(runs[0], runs[1])            # once per drawing launch
    am_site = am.noise(seed, g, col, 0)                                  # the stacked actors' site byte gives other numbers
    assert not np.any(bits(runs[0][:, OWNED]) == bits(am_site[:, OWNED]))
    actors.act(obs, noise=dev(torch, c["noise"][0]))                     # given noise is used as is, and is no draw
    assert same(host(actors.outputs["eps"])[:, OWNED], c["noise"][0][:, OWNED]) and actors.draws() == 2
    actors.act(obs, deterministic=True)                                  # draws nothing: eps = 0, raw from mu alone
    out = {k: host(v) for k, v in actors.outputs.items()}
    assert actors.draws() == 2 and not out["eps"][:, OWNED].any()
    raw, _ = model_tail(out["mu"], out["std"], out["eps"], c["obs"][0], False, deterministic=True)
    assert within_ulps(out["raw"][:, OWNED], raw[:, OWNED], 2)
    # global env indices: rows 64.. of a launch are a launch of 6 envs at replica_offset 64
    tail, _ = make(n - 64, seed=seed, replica_offset=64)
    tail.act(dev(torch, c["obs"][0, 64:]))
    assert same(host(tail.outputs["eps"])[:, OWNED], runs[0][64:, OWNED])


def test_awkward_inputs_stay_in_their_env():
    torch = pytest.importorskip("torch")
    c = setup()
    n, e0, T = 40, 35, 4
    obs = c["obs"][:T + 1, :n].copy()
    obs[1, e0, 0::5] = np.nan                                            # every agent's columns hold some of each
    obs[1, e0, 1::5] = np.inf
    obs[1, e0, 2::5] = -np.inf
    obs[1, e0, 3::5] = 3e38
    obs[1, e0, 4::5] = -3e38
    model = lm.evaluate(AGENTS, c["actors"], c["values"], obs, c["actions"][:T, :n], MIN_STD, MAX_STD)
    actors, ppo = make(n)
    log = act_steps(torch, actors, obs, c["noise"][:, :n])
    for t, got in enumerate(log):
        check_step(got, model, t, n, obs[t], c["noise"][t, :n])
        clean = c["model"]
        others = np.arange(n) != e0
        assert same(got["h"][:, others], clean["h"][:, t, :n][:, others]) and same(got["mu"][others][:, OWNED], clean["mu"][t, :n][others][:, OWNED])
    assert not np.isfinite(log[1]["mu"][e0][OWNED]).all()
    out = {k: host(v) for k, v in ppo.evaluate(dev(torch, obs), dev(torch, c["actions"][:T, :n]), want_mu_std=True).items()}
    check_seq(out, model, c["actions"][:T, :n])
    for k in ("values", "next_values"):
        others = np.arange(n) != e0
        assert same(out[k][:, others], c["model"][k][:T, :n][:, others]), k
    # (agent 0's one column holds -inf, which saturates its gates; the others hold NaN too, and a NaN state stays NaN)
    assert np.isnan(out["values"][1:, e0, 1:]).all() and np.isnan(out["next_values"][:, e0, 1:]).all() and np.isfinite(out["values"][0, e0]).all()


# ---------------------------------------------------------------------------------------------------- the sequence launch
def check_seq(out, want, actions):
    for k in ("values", "next_values", "mu", "std", "old_log_probs"):
        assert out[k].dtype == F and out[k].shape == want[k].shape, k
    assert same(out["values"], want["values"]), "values"
    assert same(out["next_values"], want["next_values"]), "next_values"
    assert same(out["mu"][..., OWNED], want["mu"][..., OWNED]), "mu"
    assert within_ulps(out["std"][..., OWNED], want["std"][..., OWNED], 1), "std"
    lp = pm.log_prob(np.asarray(actions).astype(F), out["mu"], np.where(OWNED, out["std"], 1).astype(F))
    assert within_ulps(out["old_log_probs"][..., OWNED], lp[..., OWNED], 2), "old_log_probs"


def corner(model, T, N):
    return {k: v[:T, :N] for k, v in model.items() if k not in ("h", "c")}


@pytest.mark.parametrize("n", N_ENVS)
def test_sequence_launch_equals_the_model(n):
    torch = pytest.importorskip("torch")
    c = setup()
    _, ppo = make(n)
    for T in T_SEQ:
        obs, actions = c["obs"][:T + 1, :n], c["actions"][:T, :n]
        first = ppo.evaluate(dev(torch, obs), dev(torch, actions), want_mu_std=True)          # (allocates the outputs)
        for v in first.values():
            v.fill_(SENTINEL)
        res = ppo.evaluate(dev(torch, obs), dev(torch, actions), want_mu_std=True)
        assert set(res) == {"values", "next_values", "old_log_probs", "mu", "std"} and all(res[k].data_ptr() == first[k].data_ptr() for k in res)
        out = {k: host(v).copy() for k, v in res.items()}
        check_seq(out, corner(c["model"], T, n), actions)
        for k in ("mu", "std", "old_log_probs"):
            assert np.all(out[k][..., ~OWNED] == SENTINEL), k                # columns nobody owns come back untouched
        as64 = {k: host(v) for k, v in ppo.evaluate(dev(torch, obs), dev(torch, actions.astype(np.float64)), want_mu_std=True).items()}
        for k in out:
            assert same(as64[k], out[k]), k                                  # float64 actions are read as (float)x
        assert set(ppo.evaluate(dev(torch, obs), dev(torch, actions))) == {"values", "next_values", "old_log_probs"}
    assert np.isfinite(out["old_log_probs"][..., OWNED]).all() and np.isfinite(out["values"]).all()
    assert not same(out["next_values"][:-1], out["values"][1:])         # a run of its own from a zero state


def test_stepwise_acting_equals_the_sequence_launch():
    torch = pytest.importorskip("torch")
    c = setup()
    n, T = 33, T_MAX
    actors, ppo = make(n)
    actors.reset_hidden()
    log = act_steps(torch, actors, c["obs"][:, :n], steps=T, fill=False, noise=c["noise"][:, :n])
    out = {k: host(v) for k, v in ppo.evaluate(dev(torch, c["obs"][:, :n]), dev(torch, c["actions"][:, :n]), want_mu_std=True).items()}
    for t in range(T):
        assert same(log[t]["mu"][:, OWNED], out["mu"][t][:, OWNED]) and same(log[t]["std"][:, OWNED], out["std"][t][:, OWNED]), t
        assert same(log[t]["h"], c["model"]["h"][:, t, :n]), t               # (the sequence launch keeps its h to itself: both equal the model's)


# ---------------------------------------------------------------------------------------------------- GAE with next values of their own
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("lanes", [1, 70])
def test_gae_next_equals_gae(T, lanes):
    torch = pytest.importorskip("torch")
    from pednstream_amd.rollout import gae

    rng = np.random.default_rng(10 * T + lanes)
    r, v = rng.standard_normal((T, lanes)).astype(F), rng.standard_normal((T + 1, lanes)).astype(F)
    d = (rng.random((T, lanes)) < 0.3).astype(F)
    adv0, td0 = gae(dev(torch, r), dev(torch, v), dev(torch, d), 0.99, 0.95)
    adv1, td1 = gae(dev(torch, r), dev(torch, v[:-1]), dev(torch, d), 0.99, 0.95, next_values=dev(torch, v[1:]))
    assert same(host(adv1), host(adv0)) and same(host(td1), host(td0))
    td, adv = rm.td_and_gae(r, v, d, 0.99, 0.95)
    assert same(host(td1), td) and same(host(adv1), adv)
    nv = rng.standard_normal((T, lanes)).astype(F)                       # and next values that are no shift of the values
    adv2, td2 = gae(dev(torch, r), dev(torch, v[:-1]), dev(torch, d), 0.99, 0.95, next_values=dev(torch, nv))
    td, adv = lm.gae_next(r, v[:-1], nv, d, 0.99, 0.95)
    assert same(host(td2), td) and same(host(adv2), adv)


# ---------------------------------------------------------------------------------------------------- bound modules
def test_bind_makes_the_optimiser_update_what_both_launches_read():
    torch = pytest.importorskip("torch")
    from pednstream_amd.lstm import make_actor_module, make_value_module

    c = setup()
    n, T = 3, 2
    actors, ppo = make(n)
    torch.manual_seed(4)
    amods = [actors.bind(i, make_actor_module(ow, aw).cuda()) for i, (_, ow, _, aw) in enumerate(AGENTS)]
    vmods = [ppo.bind(i, make_value_module(ow).cuda()) for i, (_, ow, _, _) in enumerate(AGENTS)]
    pads = []
    for obj in (actors, ppo):
        pad = np.ones(obj.pack_size, dtype=bool)
        for cur in obj.offsets:
            for at, shape in cur.values():
                pad[at:at + int(np.prod(shape))] = False
        pads.append(pad)
    obs, actions = c["obs"][:T + 1, :n], c["actions"][:T, :n]
    x = dev(torch, obs)

    def compare():
        for obj, mods in ((actors, amods), (ppo, vmods)):
            for i, m in enumerate(mods):
                views = obj.parameters(i)
                assert all(p.data_ptr() == views[k].data_ptr() for k, p in m.named_parameters())
        out = {k: host(v).copy() for k, v in ppo.evaluate(x, dev(torch, actions), want_mu_std=True).items()}
        asd = [{k: host(v) for k, v in m.state_dict().items()} for m in amods]
        vsd = [{k: host(v) for k, v in m.state_dict().items()} for m in vmods]
        check_seq(out, corner(lm.evaluate(AGENTS, asd, vsd, obs, actions, MIN_STD, MAX_STD), T, n), actions)
        actors.reset_hidden()
        actors.act(x[0], deterministic=True)
        assert same(host(actors.outputs["mu"])[:, OWNED], out["mu"][0][:, OWNED])          # the acting launch reads the same pack
        for i, (o0, ow, a0, aw) in enumerate(AGENTS):
            with torch.no_grad():                                        # the modules' float32 forward is the kernel's up to the summation order
                xs = x[:, :, o0:o0 + ow].transpose(0, 1).contiguous()    # an env is a batch row
                mu, std, _ = amods[i](xs[:, :T])
                v, _ = vmods[i].forward_all_steps(xs[:, :T])
                nv, _ = vmods[i].forward_all_steps(xs[:, 1:])
            t = lambda a: torch.as_tensor(a).cuda().transpose(0, 1)
            assert torch.allclose(mu, t(out["mu"][:, :, a0:a0 + aw]), rtol=1e-4, atol=1e-5), i
            assert torch.allclose(std, t(out["std"][:, :, a0:a0 + aw]), rtol=1e-4, atol=1e-5), i
            assert torch.allclose(v[:, :, 0], t(out["values"][:, :, i]), rtol=1e-4, atol=1e-5), i
            assert torch.allclose(nv[:, :, 0], t(out["next_values"][:, :, i]), rtol=1e-4, atol=1e-5), i
        for obj, pad in zip((actors, ppo), pads):
            assert not host(obj._device()["pack"])[pad].any()            # the padding is zero and stays zero
        return out

    before = compare()
    opt = torch.optim.SGD([p for m in amods + vmods for p in m.parameters()], lr=1e-2)
    for i, (o0, ow, _, _) in enumerate(AGENTS):
        xs = x[:, :, o0:o0 + ow].transpose(0, 1).contiguous()
        mu, std, _ = amods[i](xs[:, :T])
        (mu.square().sum() + std.square().sum() + vmods[i].forward_all_steps(xs[:, :T])[0].square().sum()).backward()
    opt.step()
    after = compare()
    assert not np.any(after["values"] == before["values"]) and not np.any(after["mu"][..., OWNED] == before["mu"][..., OWNED])


# ---------------------------------------------------------------------------------------------------- with an env
def make_env(name, n_envs):
    from pednstream_amd.rl_env import VecPedNetEnv

    np.random.seed(3)                  # (the scenario's demand is drawn from numpy's global stream when the network is built)
    return VecPedNetEnv(name, n_envs=n_envs, obs_mode="option3", data_dir=DATA, seed=5)


def env_rollout(torch, name, how, steps=12):
    from pednstream_amd.lstm import actor_tensor_shapes, value_tensor_shapes

    env = make_env(name, 4)
    actors = env.lstm_actors(seed=11)
    ppo = env.lstm_ppo_targets(actors)
    store = env.rollout_store(capacity=steps)
    rng = np.random.default_rng(3)
    sds = {}
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        sds[aid] = (random_sd(rng, actor_tensor_shapes(o.stop - o.start, a.stop - a.start), scale=1.0), random_sd(rng, value_tensor_shapes(o.stop - o.start), scale=1.0))
        actors.load_state_dict(aid, sds[aid][0])
        ppo.load_state_dict(aid, sds[aid][1])
    log = []
    keep = lambda: log.append({**{k: host(v).copy() for k, v in actors.outputs.items()}, "actions": host(actors.actions).copy(),
                               "h": host(actors.hidden["h"]).copy(), "c": host(actors.hidden["c"]).copy()})
    env.reset()
    store.begin()
    actors.reset_hidden()
    if how == "graph":
        roll = env.capture(lambda obs: actors.act(obs), on_step=lambda obs, rew: store.record(actors.outputs["raw"].double(), None))
        for _ in range(steps):
            roll.step()
            torch.cuda.synchronize()
            keep()
        assert roll.replays == steps - 1 and roll.eager_steps == 1 and roll.recaptures == 0
    else:
        for _ in range(steps):
            a = actors.act(env.device_views()[0])
            env.step_device(a, sync=True)
            store.record(actors.outputs["raw"].double(), None)
            torch.cuda.synchronize()
            keep()
    assert actors.draws() == steps
    assert store.finish() == steps and not store.overflow
    res = ppo.evaluate_store(store, want_mu_std=True)
    adv, td_target = ppo.compute_gae(store, res["values"], res["next_values"], 0.99, 0.95)
    torch.cuda.synchronize()
    out = {k: host(v).copy() for k, v in res.items()}
    out["adv"], out["td_target"] = host(adv).copy(), host(td_target).copy()
    v = {k: host(t).copy() for k, t in store.views().items()}
    agents, ids = ppo.agents, list(env.possible_agents)
    env.close()
    return log, out, v, agents, [sds[a] for a in ids]


@pytest.mark.parametrize("name", ["one_intersection_v0", "nine_intersections"])
def test_a_captured_env_rollout_equals_the_eager_one_and_is_evaluated(name):
    torch = pytest.importorskip("torch")
    steps = 12
    eager = env_rollout(torch, name, "eager", steps)
    log, out, v, agents, sds = env_rollout(torch, name, "graph", steps)
    for t, (a, b) in enumerate(zip(eager[0], log)):
        for k in a:
            assert same(a[k], b[k]), (t, k)                                # hidden state included
    for k in out:
        assert same(eager[1][k], out[k]), k
    for k in v:
        assert same(eager[2][k], v[k]), k
    assert not same(log[3]["eps"], log[4]["eps"]) and not same(log[0]["h"], log[5]["h"])
    # the store holds what acted, and the sequence launch reproduces the acting distribution on every row
    assert same(v["actions"], np.stack([s["raw"] for s in log]).astype(np.float64))
    for t in range(steps):
        assert same(out["mu"][t], log[t]["mu"]) and same(out["std"][t], log[t]["std"]), t
    want = lm.evaluate(agents, [a for a, _ in sds], [b for _, b in sds], v["obs"], v["actions"])
    assert same(out["values"], want["values"]) and same(out["next_values"], want["next_values"]) and same(out["mu"], want["mu"])
    assert within_ulps(out["std"], want["std"], 1)
    assert within_ulps(out["old_log_probs"], pm.log_prob(v["actions"].astype(F), out["mu"], out["std"]), 2)
    assert same(log[-1]["h"], want["h"][:, -1]) and same(log[-1]["c"], want["c"][:, -1])
    done = v["done"][:, :, None] * np.ones((1, 1, len(agents)), dtype=F)
    td, adv = lm.gae_next(v["rewards"], out["values"], out["next_values"], done, 0.99, 0.95)
    assert same(out["td_target"], td) and same(out["adv"], adv)
    assert np.isfinite(out["adv"]).all() and out["adv"].any()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    torch = pytest.importorskip("torch")
    from pednstream_amd.lstm import make_actor_module, make_value_module

    c = setup()
    n, T = 3, 2
    actors, ppo = make(n, load=False)
    obs, act = dev(torch, c["obs"][:T + 1, :n]), dev(torch, c["actions"][:T, :n])
    with pytest.raises(ValueError, match="no parameters were loaded"):
        actors.act(obs[0])
    with pytest.raises(ValueError, match="no parameters were loaded"):
        ppo.evaluate(obs, act)
    for i in range(3):
        actors.load_state_dict(i, c["actors"][i])
    with pytest.raises(ValueError, match="no value networks were loaded"):
        ppo.evaluate(obs, act)
    sd = dict(c["values"][0])
    with pytest.raises(ValueError, match="do not match"):
        ppo.load_state_dict(0, {k: v for k, v in sd.items() if k != "value_head.bias"})
    with pytest.raises(ValueError, match="do not match"):
        ppo.load_state_dict(0, {**sd, "mean_head.weight": np.zeros((1, 64), F)})
    with pytest.raises(ValueError, match="lstm.weight_hh_l0: expected shape"):
        ppo.load_state_dict(0, {**sd, "lstm.weight_hh_l0": np.zeros((128, 32), F)})
    with pytest.raises(ValueError, match="do not match"):
        actors.bind(0, make_value_module(1).cuda())
    with pytest.raises(ValueError, match="lstm.weight_ih_l0: expected shape"):
        ppo.bind(0, make_value_module(5).cuda())
    with pytest.raises(ValueError, match="mean_head.weight: expected shape"):
        actors.bind(0, make_actor_module(1, 2).cuda())
    for i, (_, ow, _, _) in enumerate(AGENTS):
        ppo.bind(i, make_value_module(ow).cuda())
    for bad in (obs[0].double(), obs[0].t().contiguous().t(), obs[0].cpu(), obs[0, :, :3].contiguous(), obs[0, :2], host(obs[0])):
        with pytest.raises(ValueError, match="obs must"):
            actors.act(bad)
    good = torch.zeros(n, N_ACTIONS, device="cuda")
    for bad in (good.double(), good.cpu(), good[:2], torch.zeros(n, 2 * N_ACTIONS, device="cuda")[:, ::2]):
        with pytest.raises(ValueError, match="noise must"):
            actors.act(obs[0], noise=bad)
    for bad in (torch.zeros(n, device="cuda"), torch.zeros(n + 1, dtype=torch.bool, device="cuda"), torch.zeros(n, dtype=torch.bool)):
        with pytest.raises(ValueError, match="mask must"):
            actors.reset_hidden(bad)
    for bad in (obs.double(), obs.transpose(0, 1).contiguous().transpose(0, 1), obs.cpu(), obs[:, :, :3].contiguous()):
        with pytest.raises(ValueError, match="obs must"):
            ppo.evaluate(bad, act)
    for bad in (act[:1], act.half(), act.cpu(), act[:, :2], act.view(T * n, N_ACTIONS), host(act)):
        with pytest.raises(ValueError, match="actions must"):
            ppo.evaluate(obs, bad)
    assert ppo.evaluate(obs, act)["values"].abs().sum().item() > 0
    with pytest.raises(ValueError, match="store must be a RolloutStore"):
        ppo.evaluate_store(obs)
    env = make_env("nine_intersections", 2)
    store = env.rollout_store(capacity=2, store_obs=False)
    env_actors = env.lstm_actors()
    with pytest.raises(ValueError, match="finish\\(\\) first"):
        env.lstm_ppo_targets(env_actors).evaluate_store(store)
    env.reset()
    store.begin()
    store.finish()
    with pytest.raises(ValueError, match="holds no rows"):
        env.lstm_ppo_targets(env_actors).evaluate_store(store)
    with pytest.raises(ValueError, match="LstmActors"):
        env.lstm_ppo_targets(env.stacked_actors("ppo", 4))
    with pytest.raises(ValueError, match="not made for this env"):
        env.lstm_ppo_targets(actors)
    with pytest.raises(ValueError, match="hidden_size 64"):
        env.lstm_actors(hidden_size=128)
    with pytest.raises(ValueError, match="num_layers 1"):
        env.lstm_actors(num_layers=2)
    env.close()
