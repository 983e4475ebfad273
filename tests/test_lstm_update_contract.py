"""DESIGN section 21 on the CPU: tests/lstm_update_model.py (the numpy restatement of pedn_lstm_grad.hpp's contract) against float64 and
float32 twins of ``make_actor_module`` / ``make_value_module`` under torch autograd, held to section 18's 4x rule, max|model - ref64| <= 4
max|ref32 - ref64| per pool (gradients per network; the forward tensors with the scalars), and the model's own properties: the two bias
gradients are the same bits, a row's through-time numbers depend on its own env only, T = 1 has no recurrent term, the Adam steps and the
early stop, begin_update, rows behind R.  The twins are built here from seeds, with parameter scales that saturate some gates.

Then the model against recordings of the reference's own ``PPOAgent(use_stacked_obs=False).update()`` (tests/golden/lstmup_*.npz,
tools/gen_lstm_update_goldens.py) under the same rule, pooled as tests/test_ppo_update_contract.py pools.
"""
import glob
import json
import os

import numpy as np
import pytest

import lstm_update_model as lum

torch = pytest.importorskip("torch")
from pednstream_amd import lstm  # noqa: E402

F = np.float32
AGENTS = [(0, 4, 0, 2), (5, 3, 2, 1)]          # (obs0, obs_w, act0, act_w) with a gap between the observation columns
N_OBS, N_ACT = 9, 3
T, N = 7, 5                                    # 35 rows: two tiles, the second of 3 rows


def modules(seed, scale=1.0):
    torch.manual_seed(seed)
    actors = [lstm.make_actor_module(ow, aw) for (_, ow, _, aw) in AGENTS]
    values = [lstm.make_value_module(ow) for (_, ow, _, _) in AGENTS]
    with torch.no_grad():
        for m in actors + values:
            m.lstm.weight_ih_l0.mul_(scale * 6.0)          # some gates beyond 0.99 / below 0.01: the backward's saturated branch
            m.lstm.bias_ih_l0.add_(torch.linspace(-2.5, 2.5, 256))
    return actors, values


def sds(mods):
    return [{k: v.detach().numpy().copy() for k, v in m.state_dict().items()} for m in mods]


def inputs(seed, T=T, N=N):
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((T + 1, N, N_OBS)).astype(F)
    act = rng.standard_normal((T, N, N_ACT)).astype(F)
    adv = rng.standard_normal((T, N, len(AGENTS))).astype(F)
    td = rng.standard_normal((T, N, len(AGENTS))).astype(F)
    return obs, act, adv, td


def old_log_probs(actors, obs, act, shift_seed):
    """evaluate's log-probabilities moved by -0.4 .. +0.2, so that ratios fall inside and beyond the clip range (and, where the shift is 0,
    are exactly 1)"""
    ev = lum.lm.evaluate(AGENTS, sds(actors), [None] * len(AGENTS), obs, act)
    rng = np.random.default_rng(shift_seed)
    shift = rng.uniform(-0.4, 0.2, ev["old_log_probs"].shape).astype(F)          # (mean(logp - old) is about +0.075: approx_kl is positive)
    shift[rng.random(shift.shape) < 0.25] = 0
    return (ev["old_log_probs"] + shift).astype(F), ev


def twin_gradients(actors, values, obs, act, old, adv, td, dtype, clip_eps=0.2):
    """per agent: {actor: {key: grad}, value: {...}, log_probs, values, actor_loss, critic_loss, approx_kl} with torch autograd in dtype"""
    res = []
    tt = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    for i, (o0, ow, a0, aw) in enumerate(AGENTS):
        import copy

        actor, value = copy.deepcopy(actors[i]).to(dtype), copy.deepcopy(values[i]).to(dtype)
        x = tt(obs[:-1, :, o0:o0 + ow]).transpose(0, 1)                 # [N, T, obs_w]: a batch is an env
        a, o = tt(act[:, :, a0:a0 + aw]).transpose(0, 1), tt(old[:, :, a0:a0 + aw]).transpose(0, 1)
        A, target = tt(adv[:, :, i]).transpose(0, 1).unsqueeze(-1), tt(td[:, :, i]).transpose(0, 1).unsqueeze(-1)
        mu, std, _ = actor(x)
        lp = torch.distributions.Normal(mu, std).log_prob(a)
        ratio = torch.exp((lp - o).clamp(-20, 20))
        actor_loss = torch.mean(-torch.min(ratio * A, torch.clamp(ratio, 1 - clip_eps, 1 + clip_eps) * A))
        v, _ = value.forward_all_steps(x)
        critic_loss = torch.mean(torch.nn.functional.mse_loss(v, target))
        actor_loss.backward()
        critic_loss.backward()
        g = lambda m: {k: p.grad.double().numpy() for k, p in m.named_parameters()}
        res.append({"actor": g(actor), "value": g(value), "log_probs": lp.detach().double().transpose(0, 1).numpy(),
                    "values": v.detach().double()[:, :, 0].transpose(0, 1).numpy(), "actor_loss": float(actor_loss.detach()), "critic_loss": float(critic_loss.detach()),
                    "approx_kl": float((lp - o).mean().detach())})
    return res


def pools(r):
    flat = lambda g: np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for _, v in sorted(g.items())])
    return {"actor": flat(r["actor"]), "value": flat(r["value"]),
            "forward": np.concatenate([np.asarray(r[k], dtype=np.float64).reshape(-1) for k in ("log_probs", "values", "actor_loss", "critic_loss", "approx_kl")])}


@pytest.fixture(scope="module")
def case():
    actors, values = modules(3)
    obs, act, adv, td = inputs(4)
    old, ev = old_log_probs(actors, obs, act, 5)
    ref64 = twin_gradients(actors, values, obs, act, old, adv, td, torch.float64)
    ref32 = twin_gradients(actors, values, obs, act, old, adv, td, torch.float32)
    return {"actors": actors, "values": values, "obs": obs, "act": act, "adv": adv, "td": td, "old": old, "ev": ev, "ref64": ref64, "ref32": ref32}


def model_gradients(c, groups, **kw):
    ep = lum.Epochs(AGENTS, sds(c["actors"]), sds(c["values"]))
    return ep.gradients(c["obs"], c["act"], c["old"], c["adv"], c["td"], groups=groups, **kw)


@pytest.fixture(scope="module")
def by_groups(case):
    return {g: model_gradients(case, g) for g in (1, 2, 3, None)}


@pytest.mark.parametrize("groups", [1, 2, 3, None])
def test_model_meets_the_4x_rule_against_the_float64_twin(case, by_groups, groups):
    res = by_groups[groups]
    for i, r in enumerate(res):
        assert (r["class"] == 0).any() and (r["class"] == 1).any() and (r["class"] == 2).any()      # ratios inside, passed and blocked
        gates = np.concatenate([r["gates"][n][k].reshape(-1) for n in ("actor", "value") for k in "ifo"])
        assert (gates > 0.99).any() and (gates < 0.01).any()
        m, r32, r64 = pools(r), pools(case["ref32"][i]), pools(case["ref64"][i])
        for name in m:
            err, ref = np.abs(m[name] - r64[name]).max(), np.abs(r32[name] - r64[name]).max()
            print(f"agent {i} groups {groups} {name}: model {err:.3e} float32 twin {ref:.3e} ratio {err / ref:.2f}")
            assert err <= 4 * ref, (i, name, err, ref)


def test_groups_change_the_order_of_sums_only(by_groups):
    a, b = by_groups[1], by_groups[3]
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["a_actor"], rb["a_actor"]) and np.array_equal(ra["log_probs"], rb["log_probs"])
        np.testing.assert_allclose(ra["actor"]["lstm.weight_hh_l0"], rb["actor"]["lstm.weight_hh_l0"], rtol=0, atol=1e-6)
    assert all(np.array_equal(x["actor"][k], y["actor"][k]) for x, y in zip(by_groups[2], by_groups[None]) for k in x["actor"])      # 2 tiles: G = 2 either way


def test_both_bias_gradients_are_the_same_bits(by_groups):
    for r in by_groups[2]:
        for n in ("actor", "value"):
            assert r[n]["lstm.bias_ih_l0"].tobytes() == r[n]["lstm.bias_hh_l0"].tobytes()
            assert np.abs(r[n]["lstm.bias_ih_l0"]).max() > 0


def test_forward_is_evaluates_and_unshifted_ratios_are_exactly_one(case):
    ep = lum.Epochs(AGENTS, sds(case["actors"]), sds(case["values"]))
    res = ep.gradients(case["obs"], case["act"], case["ev"]["old_log_probs"], case["adv"], case["td"], groups=2)
    ev = lum.lm.evaluate(AGENTS, sds(case["actors"]), sds(case["values"]), case["obs"], case["act"])
    for i, ((_, _, a0, aw), r) in enumerate(zip(AGENTS, res)):
        assert r["log_probs"].tobytes() == ev["old_log_probs"][:, :, a0:a0 + aw].tobytes()
        assert r["values"].tobytes() == ev["values"][:, :, i].tobytes()
        assert float(r["approx_kl"]) == 0.0 and (r["class"] == 0).all()


def test_a_row_depends_on_its_own_env_only(case):
    """env 3 alone (N = 1, at position 0) gives the bits it gives among the five: log_probs, values and its rows of a"""
    full = model_gradients(case, 2)
    one = {k: (v[:, 3:4] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    ep = lum.Epochs(AGENTS, sds(case["actors"]), sds(case["values"]))
    # (R differs, and with it the mean's weight: hand the full run's tail in, as a staged comparison does)
    stage = {k: np.zeros((T, 1, N_ACT), dtype=F) for k in ("d_mu", "d_z")}
    for (_, _, a0, aw), r in zip(AGENTS, full):
        stage["d_mu"][:, :, a0:a0 + aw], stage["d_z"][:, :, a0:a0 + aw] = (r[k].reshape(T, N, aw)[:, 3:4] for k in ("d_mu", "d_z"))
    alone = ep.gradients(one["obs"], one["act"], one["old"], one["adv"], one["td"], groups=2, stages=stage)
    for r, s in zip(full, alone):
        env3 = lambda v: v.reshape(T, N, -1)[:, 3]
        assert np.array_equal(env3(r["log_probs"]), s["log_probs"]) and np.array_equal(env3(r["values"]), s["values"].reshape(T, 1))
        assert np.array_equal(env3(r["a_actor"]), s["a_actor"]) and np.abs(s["a_actor"]).max() > 0      # (the value's dv carries 2 / R)


def test_one_step_has_no_recurrent_term(case):
    obs, act, adv, td = inputs(9, T=1, N=3)
    old, _ = old_log_probs(case["actors"], obs, act, 10)
    ep = lum.Epochs(AGENTS, sds(case["actors"]), sds(case["values"]))
    res = ep.gradients(obs, act, old, adv, td, groups=1)
    r64 = twin_gradients(case["actors"], case["values"], obs, act, old, adv, td, torch.float64)
    r32 = twin_gradients(case["actors"], case["values"], obs, act, old, adv, td, torch.float32)
    for r, a, b in zip(res, r64, r32):
        for n in ("actor", "value"):
            assert not r[n]["lstm.weight_hh_l0"].any()                  # h[-1] = +0.0 multiplies every row
            assert r[n]["lstm.weight_ih_l0"].any()
            # the forget gate's rows see c[-1] = +0.0
            assert not r[n]["lstm.bias_ih_l0"][64:128].any()
        m, p32, p64 = pools(r), pools(b), pools(a)
        for name in m:
            assert np.abs(m[name] - p64[name]).max() <= 4 * np.abs(p32[name] - p64[name]).max(), name


def test_epochs_step_stop_and_begin_update(case):
    """three epochs against torch's Adam on the float32 twins' gradients; the stop behind the step of an epoch whose approx_kl is beyond 1.5
    kl_tolerance; a stopped agent is left alone until begin_update()"""
    ep = lum.Epochs(AGENTS, sds(case["actors"]), sds(case["values"]))
    args = (case["obs"], case["act"], case["old"], case["adv"], case["td"])
    first = ep.epoch_update(*args, groups=2, kl_tolerance=1e9)
    assert ep.steps == [1, 1] and ep.flags == [0, 0]
    for i, r in enumerate(first):
        for n, lr in (("actor", 3e-4), ("value", 6e-4)):
            before = sds(case["actors"] if n == "actor" else case["values"])[i]
            for k, g in r[n + "_clipped"].items():
                # Adam's first step moves every element whose gradient is not tiny by lr against the gradient's sign
                big = np.abs(g) > 1e-4
                np.testing.assert_allclose((getattr(ep, n)[i][k] - before[k])[big], (-lr * np.sign(g))[big], rtol=2e-4, atol=5e-7)
            assert float(r[n + "_coef"]) <= 1.0 and float(r[n + "_norm"]) > 0
    kls = [abs(float(r["approx_kl"])) for r in first]
    # agent 0 stops behind the next step, agent 1 never does
    tol = float(ep.gradients(*args, groups=2)[0]["approx_kl"]) / 1.5 / 2
    assert tol > 0
    second = ep.epoch_update(*args, groups=2, kl_tolerance=tol, agents=[0])
    assert second[1] is None and ep.flags == [1, 0] and ep.steps == [2, 1] and kls[0] > 0
    frozen = {k: v.copy() for k, v in ep.actor[0].items()}
    third = ep.epoch_update(*args, groups=2, kl_tolerance=1e9)
    assert third[0] is None and ep.steps == [2, 2] and all(np.array_equal(frozen[k], ep.actor[0][k]) for k in frozen)
    ep.begin_update()
    assert ep.flags == [0, 0]
    assert ep.epoch_update(*args, groups=2, kl_tolerance=1e9)[0] is not None and ep.steps == [3, 3]


def test_nan_rows_behind_r_leave_every_result_unchanged(case):
    """the arrays go on behind the T steps that count, with NaN in every row there (up to the end of the last row tile and beyond)"""
    c = case
    pad = lambda v: np.concatenate([v, np.full((6,) + v.shape[1:], np.nan, dtype=F)])
    for i, (o0, ow, a0, aw) in enumerate(AGENTS):
        actor, value = sds(c["actors"])[i], sds(c["values"])[i]
        args = (c["obs"][:T, :, o0:o0 + ow], c["act"][:, :, a0:a0 + aw], c["old"][:, :, a0:a0 + aw], c["adv"][:, :, i], c["td"][:, :, i])
        want = lum.agent_gradients(actor, value, *args, groups=2)
        got = lum.agent_gradients(actor, value, *[pad(v) for v in args], groups=2, live=T)
        for net in ("actor", "value"):
            assert all(np.array_equal(got[net][k], want[net][k]) and np.isfinite(got[net][k]).all() for k in want[net]), net
        assert all(got[k] == want[k] for k in ("actor_loss", "critic_loss", "approx_kl"))
        assert np.array_equal(got["a_actor"], want["a_actor"]) and np.array_equal(got["log_probs"], want["log_probs"])


# ---------------------------------------------------------------------------------------------------- against the reference's update()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((4, 1), (20, 4), (56, 8), (6, 2))
SIZE_LIMIT = 666561


def load(case, name):
    with np.load(os.path.join(GOLDEN, f"lstmup_o{case[0]}_a{case[1]}_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def part(z, tag):
    return {k[len(tag) + 1:]: v for k, v in z.items() if k.startswith(tag + ".")}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "o%d_a%d" % c)
def test_the_model_meets_the_rule_against_the_references_update(case):
    """Per network, pooled over the recorded epochs: max_t(max|model_t - ref64_t| / max|ref64_t|) <= 4 max_t(max|ref32_t - ref64_t| /
    max|ref64_t|) over the clipped gradient tensors, and over the forward tensors with the single numbers (losses, approx_kl, norms), the
    epochs behind epoch 0 once more by themselves; max|model - ref64| <= 4 max|ref32 - ref64| behind Adam for the parameters, exp_avg and
    exp_avg_sq of each network and epoch; the stop flag and the number of steps are the reference's."""
    sam = lum.um.sam
    obs_dim, act_dim = case
    inp = load(case, "in")
    info = json.loads(str(inp["info_json"]))
    assert (info["obs_dim"], info["act_dim"], info["T"]) == (obs_dim, act_dim, 37)
    assert info["gates"][0] < 0.01 or info["gates"][1] > 0.99
    for path in glob.glob(os.path.join(GOLDEN, "lstmup_o%d_a%d_*.npz" % case)):
        assert os.path.getsize(path) <= SIZE_LIMIT, path
    agents = [(0, obs_dim, 0, act_dim)]
    args = (inp["obs"][:, None, :], inp["actions"][:, None, :], inp["old_log_probs"][:, None, :], inp["advantage"][:, None, None], inp["td_target"][:, None, None])
    hyper = dict(actor_lr=info["actor_lr"], critic_lr=info["critic_lr"], clip_eps=info["clip_eps"], max_grad_norm=info["max_grad_norm"],
                 kl_tolerance=info["kl_tolerance"])
    rel = lambda x, ref: float(np.max(np.abs(np.asarray(x, dtype=np.float64) - ref)) / np.max(np.abs(ref)))
    worst = {k: [0.0, 0.0] for k in ("actor gradients", "value gradients", "forward", "forward behind epoch 0")}
    prev = {"actor": None, "value": None}
    ratios = {}
    for e in range(info["epochs_run"]):
        z = {net: load(case, f"e{e}_{net}_grad") for net in ("actor", "value")}
        ad = {net: load(case, f"e{e}_{net}_adam") for net in ("actor", "value")}
        ep = lum.Epochs(agents, [part(z["actor"], "p")], [part(z["value"], "p")])
        r = ep.gradients(*args, clip_eps=hyper["clip_eps"], max_grad_norm=hyper["max_grad_norm"])[0]
        fwd = [(r["log_probs"], z["actor"], "log_probs"), (r["values"], z["value"], "values"), (r["actor_loss"], z["actor"], "loss"),
               (r["critic_loss"], z["value"], "loss"), (r["approx_kl"], z["actor"], "approx_kl"), (r["actor_norm"], z["actor"], "norm"),
               (r["value_norm"], z["value"], "norm")]
        for mine, zz, key in fwd:
            ref32 = zz[key].astype(np.float64)
            ref64 = ref32 - zz["d" + key]
            if np.max(np.abs(ref64)) == 0:
                assert np.all(np.asarray(mine) == 0), key
                continue
            # (in epoch 0 approx_kl and actor_loss are sums that cancel to nearly nothing: they decide the pool of all epochs, so the
            # epochs behind it are pooled once more by themselves)
            for name in ("forward",) + (("forward behind epoch 0",) if e else ()):
                worst[name][0] = max(worst[name][0], rel(np.asarray(mine).reshape(ref64.shape), ref64))
                worst[name][1] = max(worst[name][1], rel(ref32, ref64))
        assert F(r["actor_coef"]) == F(z["actor"]["coef"]) or abs(float(r["actor_coef"]) - float(z["actor"]["coef"])) <= 1e-5 * float(z["actor"]["coef"])
        for net, lr in (("actor", hyper["actor_lr"]), ("value", hyper["critic_lr"])):
            g32, dg = part(z[net], "g"), part(z[net], "dg")
            for key in g32:
                ref64 = g32[key].astype(np.float64) - dg[key]
                if np.max(np.abs(ref64)) == 0:
                    assert not r[net + "_clipped"][key].any(), (net, key)
                    continue
                w = worst[net + " gradients"]
                w[0], w[1] = max(w[0], rel(r[net + "_clipped"][key], ref64)), max(w[1], rel(g32[key], ref64))
            # Adam on the RECORDED float32 gradients and state, as the reference's float64 twin was stepped
            p0, post, dpost = part(z[net], "p"), part(z[net], "post"), part(z[net], "dpost")
            m1, dm, v1, dv = (part(ad[net], t) for t in ("m", "dm", "v", "dv"))
            m0, v0 = prev[net] if prev[net] is not None else ({k: np.zeros_like(x) for k, x in p0.items()},) * 2
            err = {t: [0.0, 0.0] for t in ("parameters", "exp_avg", "exp_avg_sq")}
            for key in p0:
                pm_, mm_, vm_ = sam.adam(p0[key], g32[key], m0[key], v0[key], e + 1, lr)
                for t, mine, r32, d in (("parameters", pm_, post[key], dpost[key]), ("exp_avg", mm_, m1[key], dm[key]), ("exp_avg_sq", vm_, v1[key], dv[key])):
                    ref64 = r32.astype(np.float64) - d
                    err[t][0] = max(err[t][0], float(np.max(np.abs(mine.astype(np.float64) - ref64))))
                    err[t][1] = max(err[t][1], float(np.max(np.abs(d))))
            for t, (a, b) in err.items():
                ratios[(net, t)] = max(ratios.get((net, t), 0.0), a / b if b else (0.0 if a == 0 else np.inf))
            prev[net] = (m1, v1)
    for k, (a, b) in worst.items():
        ratios[k] = a / b if b else 0.0
    print(case, {str(k): round(v, 2) for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v <= 4.0, (case, k, v)
    # the stop flag and the number of steps: the model's own chain from the first recorded parameters
    z0 = {net: load(case, f"e0_{net}_grad") for net in ("actor", "value")}
    ep = lum.Epochs(agents, [part(z0["actor"], "p")], [part(z0["value"], "p")])
    ep.begin_update()
    for _ in range(info["epochs"]):
        ep.epoch_update(*args, **hyper)
    assert ep.steps == [info["epochs_run"]] and ep.flags == [int(info["stopped"])], (ep.steps, ep.flags, info["epochs_run"], info["stopped"])
