"""The recurrent PPO agents' clipped-loss epochs on the device AT THEIR EDGES ("Edges"), against
tests/lstm_update_model.py with the allowances of tests/test_gpu_lstm_update.py and no other: bit for bit where the arithmetic is float32,
section 20's 1-4 ulps through the staged comparison.  What each test pins:

    saturated cell   lstm_sigmoid at 0.0f, 1.0f and in the subnormals, lstm_tanh at +-1, pedn_exp's branches beyond 512 and 1024, h' = +-0.0
                     in front of the backward's mask `hp > 0.0f`, the weight-gradient launch's relu and h[t - 1], subnormal a and gradients
    poison           `r < live`, `me.mine`, `r < nrows`, `sT[r] = -1`, `fresh`: NaN in the workspace, the activations, the tail, the outputs,
                     obs[T] and every column nobody owns reaches no result
    a NaN's reach    one env's NaN stays in that env's rows and that agent's sums
    the tail         d_z == 0 on the std clamp, ratios exactly on 1 +- clip_eps, d_mu == d_z == 0 beyond +-20, advantages all zero, through
                     sD, the tail planes and the backward's heads loop
    float64 actions  act_f64 = 1 against the model
    shapes           obs_w 32, 64, 65; act_w 5, 7, 8; N = 40 (a wave with live == 0); a third env tile with groups that do not divide the
                     row tiles; workspaces per shape
tests/test_lstm_update_edges_host.py proves on the CPU that these inputs reach the edges: a model that is wrong there gives other bits.
"""
import numpy as np
import pytest

import lstm_edge_cases as ec
import lstm_update_model as lum
from test_gpu_actors import host, same
from test_gpu_lstm import AGENTS, MAX_STD, MIN_STD, N_ACTIONS, N_OBS, OWNED, SENTINEL, random_sd
from test_gpu_lstm_update import check_gates, gate_gradients, inputs, make, setup
from test_gpu_ppo_update import HYPER, check_epoch, dev, padding_is_zero, staged, um_scalars

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("obs", "actions", "old", "adv", "td")
OWNED_OBS = np.zeros(N_OBS, dtype=bool)
for _o0, _ow, _, _ in AGENTS:
    OWNED_OBS[_o0:_o0 + _ow] = True


def hosted(args):
    return dict(zip(NAMES, (host(a) for a in args)))


def with_old(torch, ppo, c, T, N, old_of, actions=None):
    """inputs() with old_log_probs = old_of(evaluate's log-probabilities on the loaded parameters)"""
    obs = dev(torch, c["obs"][:T + 1, :N])
    act = dev(torch, c["actions"][:T, :N]) if actions is None else actions
    old = dev(torch, old_of(host(ppo.evaluate(obs, act)["old_log_probs"])))
    return obs, act, old, dev(torch, c["adv"][:T, :N]), dev(torch, c["td"][:T, :N])


def model_of(ppo, args, model, groups, update=False):
    ah = hosted(args)
    run = model.epoch_update if update else model.gradients
    return run(ah["obs"], ah["actions"], ah["old"], ah["adv"], ah["td"], groups=groups, stages=staged(ppo), **(HYPER if update else {})), ah


def snapshot(ppo, T, N, groups, n_agents=len(AGENTS)):
    """host copies of everything an epoch_gradients call leaves: per agent's columns where a column has an owner"""
    o = ppo.epoch_outputs
    s = {k: host(getattr(o, k)).copy() for k in ("log_probs", "values", "std", "d_mu", "d_z") + tuple(um_scalars())}
    for i in range(n_agents):
        for net in ("actor", "value"):
            for key, v in o.grads(i, net, clipped=False).items():
                s[("raw", i, net, key)] = host(v).copy()
    s["a"] = gate_gradients(ppo, T, N, groups).copy()
    return s


def agent_part(s, i, agents=AGENTS):
    """what of a snapshot belongs to agent i"""
    _, _, a0, aw = agents[i]
    part = {k: s[k][:, :, a0:a0 + aw] for k in ("log_probs", "std", "d_mu", "d_z")}
    part["values"] = s["values"][:, :, i]
    part.update({k: s[k][i] for k in um_scalars()})
    part.update({k: v for k, v in s.items() if isinstance(k, tuple) and k[1] == i})
    part["a"] = s["a"][:, i]
    return part


def differing(a, b):
    return [k for k in a if not same(a[k], b[k])]


# ---------------------------------------------------------------------------------------------------- the ends of the cell
@pytest.mark.parametrize("T,N,groups", [(4, 5, 2), (3, 33, 2)])
def test_saturated_cell_equals_the_model(T, N, groups):
    torch = pytest.importorskip("torch")
    c = setup()
    actors, values = ec.doctored(c)
    ppo = make()
    for i in range(len(AGENTS)):
        ppo.actors.load_state_dict(i, actors[i])
        ppo.load_state_dict(i, values[i])
    model = lum.Epochs(AGENTS, actors, values, MIN_STD, MAX_STD)
    args = with_old(torch, ppo, c, T, N, lambda logp: ec.shifted(logp, c["shift"][:T, :N]))
    what = ("saturated", T, N, groups)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    res, ah = model_of(ppo, args, model, groups)
    for i, r in enumerate(res):                                   # first, so that the case cannot go vacuous
        for net in ("actor", "value"):
            missed = [k for k, ok in ec.edge_conditions(r["gates"][net]).items() if not ok]
            assert not missed, (what, i, net, missed)
    check_epoch(ppo, model, res, ah, what + ("gradients",), stepped=False)
    check_gates(ppo, res, T, N, groups, what)
    a = gate_gradients(ppo, T, N, groups)
    kept = host(ppo._uout[(T, N, groups)]["act"])[:, :, :, :128]   # h', c' as the forward left them: signed zeros and subnormals included
    for i, r in enumerate(res):
        for z, net in enumerate(("value", "actor")):
            fw = r["gates"][net]
            assert same(kept[z, i, :, :64], fw["h"].reshape(T * N, 64)) and same(kept[z, i, :, 64:], fw["c"].reshape(T * N, 64)), (what, "h', c'", i, net)
            sub = ec.subnormal(r["a_" + net])
            assert sub.any() and same(a[z, i][sub], r["a_" + net][sub]), (what, "subnormal a", i, net)
            got = {k: host(v) for k, v in ppo.epoch_outputs.grads(i, net, clipped=False).items()}
            subs = 0
            for key in lum.LSTM_KEYS:
                sub = ec.subnormal(r[net][key])
                subs += int(sub.sum())
                assert same(got[key][sub], r[net][key][sub]), (what, "subnormal gradient", i, net, key)
            assert subs > 0, (what, "no subnormal LSTM gradient", i, net)
    for epoch in range(2):
        ppo.epoch_update(*args, groups=groups, want_tail=True, **HYPER)
        res, ah = model_of(ppo, args, model, groups, update=True)
        check_epoch(ppo, model, res, ah, what + ("epoch", epoch), stepped=True)
        check_gates(ppo, res, T, N, groups, what + ("epoch", epoch))
    assert padding_is_zero(ppo), what


# ---------------------------------------------------------------------------------------------------- the guards
def test_poison_reaches_no_result():
    """The workspace, the activations, the tail and the outputs are allocated as zeros once per shape and used again: a read of a row, slab
    or plane that should not be read would find zeros or last epoch's numbers and pass.  Here it finds NaN."""
    torch = pytest.importorskip("torch")
    T, N, groups = 5, 13, 2
    c = setup()
    ppo = make()
    hidden = ppo.actors.hidden
    hidden["h"].fill_(SENTINEL)
    hidden["c"].fill_(SENTINEL / 2)
    args = inputs(torch, ppo, c, T, N)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    first = snapshot(ppo, T, N, groups)
    nan = float("nan")
    out = ppo._uout[(T, N, groups)]
    assert out["ws"].shape[0] == 2
    for k in ("ws", "act", "tail4", "log_probs", "values"):
        out[k].fill_(nan)
    obs, act, old, adv, td = (a.clone() for a in args)
    obs[T] = nan                                                  # the frame behind the last step
    obs[:, :, dev(torch, ~OWNED_OBS)] = nan
    act[:, :, dev(torch, ~OWNED)] = nan
    old[:, :, dev(torch, ~OWNED)] = nan                           # (advantages and td_target have a column per agent and none without an owner)
    ppo.epoch_gradients(obs, act, old, adv, td, groups=groups, want_tail=True)
    second = snapshot(ppo, T, N, groups)
    for i in range(len(AGENTS)):
        assert not differing(agent_part(first, i), agent_part(second, i)), (i, differing(agent_part(first, i), agent_part(second, i)))
        assert all(np.isfinite(v).all() for v in agent_part(second, i).values()), i
    for k in ("log_probs", "std", "d_mu", "d_z"):
        assert np.isnan(second[k][:, :, ~OWNED]).all(), (k, "a column nobody owns was written")
    # the epochs start from a zero state of their own: the acting state is neither read (above) nor written
    ppo.epoch_update(*args, groups=groups, **HYPER)
    assert (host(ppo.actors.hidden["h"]) == F(SENTINEL)).all() and (host(ppo.actors.hidden["c"]) == F(SENTINEL / 2)).all()
    assert ppo.adam_steps() == [1] * len(AGENTS)


def test_a_nan_stays_in_its_env_and_its_agent():
    torch = pytest.importorskip("torch")
    T, N, groups, who, env, step = 5, 13, 2, 1, 7, 2
    c = setup()
    ppo = make()
    args = inputs(torch, ppo, c, T, N)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    first = snapshot(ppo, T, N, groups)
    obs = args[0].clone()
    obs[step, env, AGENTS[who][0] + 4] = float("nan")
    ppo.epoch_gradients(obs, *args[1:], groups=groups, want_tail=True)
    second = snapshot(ppo, T, N, groups)
    for i in (0, 2):
        assert not differing(agent_part(first, i), agent_part(second, i)), (i, differing(agent_part(first, i), agent_part(second, i)))
    was, now = agent_part(first, who), agent_part(second, who)
    hit = np.zeros((T, N), dtype=bool)
    hit[step:, env] = True
    for k in ("log_probs", "values"):
        assert np.isnan(now[k][hit]).all() and np.isfinite(now[k][~hit]).all() and same(now[k][~hit], was[k][~hit]), k
    others = np.arange(N) != env
    rows = lambda a: a.reshape(2, T, N, 256)[:, :, others]
    assert same(rows(now["a"]), rows(was["a"])) and np.abs(rows(was["a"])).max() > 0
    for k, v in now.items():
        if isinstance(k, tuple):
            assert not np.isfinite(v).any(), (k, "a gradient of the agent whose env holds a NaN is finite")
    assert ppo.adam_steps() == [0] * len(AGENTS)


# ---------------------------------------------------------------------------------------------------- the loss' tail through the recurrent routing
def test_std_on_its_clamp_bounds():
    torch = pytest.importorskip("torch")
    T, N, groups, lo, hi = 6, 13, 2, 0.4, 1.2      # (softplus passes 1.2 at step 5 of env 11, and lies under 0.4 from step 0 on)
    c = setup()
    ppo = make(min_std=lo, max_std=hi)
    model = lum.Epochs(AGENTS, c["actors"], c["values"], lo, hi)
    args = inputs(torch, ppo, c, T, N)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    res, ah = model_of(ppo, args, model, groups)
    std, d_z = host(ppo.epoch_outputs.std)[:, :, OWNED], host(ppo.epoch_outputs.d_z)[:, :, OWNED]
    assert (std == F(lo)).any() and (std == F(hi)).any() and ((std > F(lo)) & (std < F(hi))).any()
    check_epoch(ppo, model, res, ah, "std bounds", stepped=False)
    check_gates(ppo, res, T, N, groups, "std bounds")
    assert (d_z[(std == F(lo)) | (std == F(hi))] == 0).all() and (d_z != 0).any()


def test_ratios_exactly_on_the_clip_bounds():
    torch = pytest.importorskip("torch")
    T, N, groups = 5, 13, 2
    c = setup()
    ppo = make()
    model = lum.Epochs(AGENTS, c["actors"], c["values"], MIN_STD, MAX_STD)
    args = with_old(torch, ppo, c, T, N, ec.on_clip_bounds)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    res, ah = model_of(ppo, args, model, groups)
    check_epoch(ppo, model, res, ah, "clip bounds", stepped=False)
    check_gates(ppo, res, T, N, groups, "clip bounds")
    ratio = np.exp((host(ppo.epoch_outputs.log_probs) - ah["old"]).astype(np.float64)).astype(F)[:, :, OWNED]
    assert (ratio[0] == F(1.2)).any() and (ratio[1] == F(0.8)).any(), "no ratio landed exactly on a bound"


def test_log_ratios_beyond_twenty_pass_nothing():
    torch = pytest.importorskip("torch")
    T, N, groups = 5, 13, 2
    c = setup()
    ppo = make()
    model = lum.Epochs(AGENTS, c["actors"], c["values"], MIN_STD, MAX_STD)
    args = with_old(torch, ppo, c, T, N, ec.beyond_twenty)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    res, ah = model_of(ppo, args, model, groups)
    dl = (host(ppo.epoch_outputs.log_probs) - ah["old"])[:, :, OWNED]
    assert (dl[0] > 20).all() and (dl[1] < -20).all() and (np.abs(dl[2:]) < 20).all()
    d_mu, d_z = host(ppo.epoch_outputs.d_mu)[:, :, OWNED], host(ppo.epoch_outputs.d_z)[:, :, OWNED]
    assert (d_mu[:2] == 0).all() and (d_z[:2] == 0).all() and (d_mu[2:] != 0).any() and (d_z[2:] != 0).any()
    check_epoch(ppo, model, res, ah, "beyond +-20", stepped=False)
    check_gates(ppo, res, T, N, groups, "beyond +-20")


def test_zero_advantages_give_no_actor_gradient():
    torch = pytest.importorskip("torch")
    T, N, groups = 5, 13, 2
    c = setup()
    ppo = make()
    model = lum.Epochs(AGENTS, c["actors"], c["values"], MIN_STD, MAX_STD)
    obs, act, old, adv, td = inputs(torch, ppo, c, T, N)
    args = (obs, act, old, torch.zeros_like(adv), td)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    res, ah = model_of(ppo, args, model, groups)
    o = ppo.epoch_outputs
    assert (host(o.actor_norm) == 0).all() and (host(o.actor_coef) == 1).all() and (host(o.actor_loss) == 0).all()
    a = gate_gradients(ppo, T, N, groups)
    for i, r in enumerate(res):
        assert all((host(v) == 0).all() for v in o.grads(i, "actor", clipped=False).values()), i
        assert all((host(v) == 0).all() for v in o.grads(i, "actor").values()), i
        assert (a[1, i] == 0).all() and same(a[1, i], r["a_actor"]), i                        # +-0.0, the model's signs
        assert same(a[0, i], r["a_value"]) and np.abs(a[0, i]).max() > 0, i
    check_epoch(ppo, model, res, ah, "zero advantages", stepped=False)


# ---------------------------------------------------------------------------------------------------- float64 actions
def test_float64_actions_equal_the_model_and_their_float32_rounding():
    torch = pytest.importorskip("torch")
    T, N, groups = 5, 13, 2
    c = setup()
    ppo = make()
    model = lum.Epochs(AGENTS, c["actors"], c["values"], MIN_STD, MAX_STD)
    act64 = (dev(torch, c["actions"][:T, :N]).double() + 1e-9).contiguous()
    assert not same(host(act64), host(act64.float()).astype(np.float64))                       # not float32 numbers
    args = with_old(torch, ppo, c, T, N, lambda logp: ec.shifted(logp, c["shift"][:T, :N]), actions=act64)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    res, ah = model_of(ppo, args, model, groups)
    assert ah["actions"].dtype == np.float64
    check_epoch(ppo, model, res, ah, "float64 actions", stepped=False)
    check_gates(ppo, res, T, N, groups, "float64 actions")
    first = snapshot(ppo, T, N, groups)
    ppo.epoch_gradients(args[0], act64.float().contiguous(), *args[2:], groups=groups, want_tail=True)
    second = snapshot(ppo, T, N, groups)
    for i in range(len(AGENTS)):
        assert not differing(agent_part(first, i), agent_part(second, i)), (i, differing(agent_part(first, i), agent_part(second, i)))


# ---------------------------------------------------------------------------------------------------- shapes
_wide = {}


def wide_setup():
    if not _wide:
        from pednstream_amd.lstm import actor_tensor_shapes, value_tensor_shapes

        rng = np.random.default_rng(2111)
        T, N, w = 3, 70, _wide
        w["actors"] = [random_sd(rng, actor_tensor_shapes(ow, aw)) for (_, ow, _, aw) in ec.WIDE_AGENTS]
        w["values"] = [random_sd(rng, value_tensor_shapes(ow)) for (_, ow, _, _) in ec.WIDE_AGENTS]
        w["obs"] = (rng.standard_normal((T + 1, N, ec.WIDE_N_OBS)) * 2 + 1).astype(F)
        w["actions"] = (rng.standard_normal((T, N, ec.WIDE_N_ACTIONS)) * 1.5).astype(F)
        w["adv"] = rng.standard_normal((T, N, len(ec.WIDE_AGENTS))).astype(F)
        w["td"] = rng.standard_normal((T, N, len(ec.WIDE_AGENTS))).astype(F)
        w["shift"] = (rng.standard_normal((T, N, ec.WIDE_N_ACTIONS)) * 0.25).astype(F)
    return _wide


def wide_make():
    pytest.importorskip("torch")
    from pednstream_amd.lstm import LstmActors, LstmPpoTargets

    w = wide_setup()
    actors = LstmActors(ec.WIDE_AGENTS, np.zeros(ec.WIDE_N_ACTIONS, dtype=F), np.full(ec.WIDE_N_ACTIONS, 4.0, dtype=F), 1, ec.WIDE_N_OBS,
                        ec.WIDE_N_ACTIONS, delta_actions=False, min_std=MIN_STD, max_std=MAX_STD)
    ppo = LstmPpoTargets(actors)
    for i in range(len(ec.WIDE_AGENTS)):
        actors.load_state_dict(i, w["actors"][i])
        ppo.load_state_dict(i, w["values"][i])
    return ppo


@pytest.mark.parametrize("T,N,groups", [(2, 40, 2), (3, 70, 3)])
def test_wide_agents_equal_the_model(T, N, groups):
    """(2, 40, 2): 80 rows, three row tiles for two groups, and wave 1 of the second env tile starts AT env 40: live == 0.  (3, 70, 3): a
    third env tile of 6 envs, seven row tiles for three groups."""
    torch = pytest.importorskip("torch")
    w = wide_setup()
    ppo = wide_make()
    model = lum.Epochs(ec.WIDE_AGENTS, w["actors"], w["values"], MIN_STD, MAX_STD)
    args = inputs(torch, ppo, w, T, N)
    what = ("wide", T, N, groups)
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    res, ah = model_of(ppo, args, model, groups)
    check_epoch(ppo, model, res, ah, what + ("gradients",), stepped=False)
    check_gates(ppo, res, T, N, groups, what)
    ppo.epoch_update(*args, groups=groups, want_tail=True, **HYPER)
    res, ah = model_of(ppo, args, model, groups, update=True)
    check_epoch(ppo, model, res, ah, what + ("epoch",), stepped=True)
    check_gates(ppo, res, T, N, groups, what + ("epoch",))
    assert padding_is_zero(ppo), what


def test_a_second_shape_leaves_the_first_shapes_results():
    """the workspaces are per (T, N, groups), the gradient packs and the Adam state shared: nothing of one shape's call lasts into another's"""
    torch = pytest.importorskip("torch")
    w = wide_setup()
    ppo = wide_make()
    shapes = ((2, 40, 2), (3, 70, 3))
    args = [inputs(torch, ppo, w, T, N) for (T, N, _) in shapes]
    snaps = []
    for k in (0, 1, 0):
        T, N, groups = shapes[k]
        ppo.epoch_gradients(*args[k], groups=groups, want_tail=True)
        snaps.append(snapshot(ppo, T, N, groups, len(ec.WIDE_AGENTS)))
    assert set(ppo._uout) == set(shapes)
    for i in range(len(ec.WIDE_AGENTS)):
        a, b = agent_part(snaps[0], i, ec.WIDE_AGENTS), agent_part(snaps[2], i, ec.WIDE_AGENTS)
        assert not differing(a, b), (i, differing(a, b))
        other = agent_part(snaps[1], i, ec.WIDE_AGENTS)
        assert any(not same(other[k], b[k]) for k in b if isinstance(k, tuple))                # (the other shape's call did write the shared packs)
    assert ppo.adam_steps() == [0] * len(ec.WIDE_AGENTS)
