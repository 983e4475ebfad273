"""The numpy model of PPO's clipped-loss epochs (tests/ppo_update_model.py) against recordings of the reference's own
PPOAgent.update() (tests/golden/ppoup_*.npz, tools/gen_ppo_update_goldens.py) under section 18's rule with the factor 4, and by itself: the
numbers of groups, a row's independence of its position, rows behind the batch, the stop."""
import glob
import json
import os

import numpy as np
import pytest

import sac_actor_model as sam

import ppo_eval_model as pm
import ppo_update_model as um

F = np.float32
OBS_W, ACT_W, S, T = 20, 4, 5, 37          # section 16's second shape; 37 rows are two tiles, the second of 5
AGENTS = [(0, OBS_W, 0, ACT_W)]


def random_sd(rng, shapes, scale=1.0):
    sd = {}
    for key, shape in shapes:
        fan = shape[-1] if len(shape) == 2 else 64
        sd[key] = (rng.uniform(-1, 1, size=shape) * scale / np.sqrt(fan)).astype(F)
        if key == "ln.weight":
            sd[key] = (1.0 + 0.1 * rng.uniform(-1, 1, size=shape)).astype(F)
    return sd


@pytest.fixture(scope="module")
def case():
    from pednstream_amd.policy import tensor_shapes
    from pednstream_amd.ppo import value_tensor_shapes

    rng = np.random.default_rng(20)
    actor, value = random_sd(rng, tensor_shapes("ppo", OBS_W, ACT_W, S)), random_sd(rng, value_tensor_shapes(OBS_W, S))
    obs = rng.standard_normal((T + 1, 1, OBS_W)).astype(F)
    ev = pm.evaluate(AGENTS, [actor], [value], obs, np.zeros((T, 1, ACT_W), dtype=F), S)
    act = (ev["mu"] + ev["std"] * rng.standard_normal((T, 1, ACT_W)).astype(F)).astype(F)      # samples of the policy, as a rollout's are
    logp = pm.evaluate(AGENTS, [actor], [value], obs, act, S)["old_log_probs"]
    old = (logp + (rng.standard_normal((T, 1, ACT_W)) * 0.25).astype(F)).astype(F)
    adv, td = rng.standard_normal((T, 1, 1)).astype(F), rng.standard_normal((T, 1, 1)).astype(F)
    return dict(actor=actor, value=value, obs=obs, act=act, old=old, adv=adv, td=td, logp=logp)


def epochs(c):
    return um.Epochs(AGENTS, [c["actor"]], [c["value"]], S)


def test_groups_change_the_order_only_and_meet_the_rule_against_a_float64_twin(case):
    torch = pytest.importorskip("torch")
    from pednstream_amd.policy import make_module
    from pednstream_amd.ppo import make_value_module

    c = case
    x = pm.stacks(c["obs"], S)[:T].reshape(T, S, OBS_W)
    ref = {}
    for dt in (torch.float32, torch.float64):
        a, v = make_module("ppo", OBS_W, ACT_W, S).to(dt), make_value_module(OBS_W, S).to(dt)
        a.load_state_dict({k: torch.as_tensor(w).to(dt) for k, w in c["actor"].items()})
        v.load_state_dict({k: torch.as_tensor(w).to(dt) for k, w in c["value"].items()})
        t = lambda w: torch.as_tensor(w).to(dt)
        mu, std = a(t(x))
        lp = torch.distributions.Normal(mu, std).log_prob(t(c["act"][:, 0]))
        ratio = torch.exp((lp - t(c["old"][:, 0])).clamp(-20, 20))
        A = t(c["adv"][:, 0])
        al = torch.mean(-torch.min(ratio * A, torch.clamp(ratio, 1 - 0.2, 1 + 0.2) * A))
        cl = torch.mean(torch.nn.functional.mse_loss(v(t(x)), t(c["td"][:, 0])))
        al.backward()
        cl.backward()
        ref[dt] = {"actor": {k: p.grad.numpy().astype(np.float64) for k, p in a.named_parameters()},
                   "value": {k: p.grad.numpy().astype(np.float64) for k, p in v.named_parameters()},
                   "ratio": ratio.detach().numpy()}
    r32, r64 = ref[torch.float32], ref[torch.float64]
    inside = lambda r, lo, hi: (r >= lo) & (r <= hi)
    assert (inside(r32["ratio"], F(0.8), F(1.2)) == inside(r64["ratio"], 0.8, 1.2)).all()       # every element in the same class in both
    seen = []
    for groups in (1, 2, 3, None):
        r = epochs(c).gradients(c["obs"], c["act"], c["old"], c["adv"], c["td"], groups=groups)[0]
        assert set(np.unique(r["class"])) == {0, 1, 2}                                      # ties, passed and blocked elements all occur
        assert ((r["class"] == 0) == inside(r64["ratio"], 0.8, 1.2)).all()
        for net in ("actor", "value"):
            err = lambda g: max(np.abs(g[k] - r64[net][k]).max() / np.abs(r64[net][k]).max() for k in r64[net])
            ratio = err(r[net]) / err(r32[net])
            print(f"groups {groups} {net}: model / float32 torch = {ratio:.2f}")
            assert ratio <= 4.0, (groups, net, ratio)
        seen.append(r)
    # two tiles: one group is another order of the same two partials than two; more groups than tiles change nothing
    assert all(np.array_equal(seen[1]["actor"][k], seen[3]["actor"][k]) for k in seen[1]["actor"])
    assert all(np.array_equal(seen[0]["log_probs"], s["log_probs"]) and np.array_equal(seen[0]["values"], s["values"]) for s in seen)
    # clip_grad_norm_: the coefficient scales here (the actor's norm is above 0.5) and leaves alone when the bound is generous
    assert seen[0]["actor_coef"] < 1 and um.clip(seen[0]["actor"], um.order(um.ACTOR_KEYS), 1e3)[1] == 1


def test_a_rows_forward_depends_on_its_own_frames_only(case):
    c = case
    whole = epochs(c).gradients(c["obs"], c["act"], c["old"], c["adv"], c["td"], groups=2)[0]
    T2 = 9
    part = epochs(c).gradients(c["obs"][:T2 + 1], c["act"][:T2], c["old"][:T2], c["adv"][:T2], c["td"][:T2], groups=1)[0]
    for k in ("log_probs", "values", "mu", "std"):
        assert np.array_equal(part[k], whole[k][:T2]), k
    # as two envs of other times: the rows of env 1 are those of a rollout of its own
    obs2 = np.concatenate([c["obs"][:T2 + 1], c["obs"][T2 + 1:2 * T2 + 2]], axis=1)
    two = epochs(c).gradients(obs2, np.concatenate([c["act"][:T2], c["act"][:T2]], axis=1), np.concatenate([c["old"][:T2]] * 2, axis=1),
                              np.concatenate([c["adv"][:T2]] * 2, axis=1), np.concatenate([c["td"][:T2]] * 2, axis=1), groups=3)[0]
    assert np.array_equal(two["values"].reshape(T2, 2)[:, 0], whole["values"][:T2])
    assert np.array_equal(two["log_probs"].reshape(T2, 2, ACT_W)[:, 0], whole["log_probs"][:T2])
    # before any step log_probs are evaluate's bits: with them as old_log_probs every ratio is exactly 1 and approx_kl exactly 0
    same = epochs(c).gradients(c["obs"], c["act"], c["logp"], c["adv"], c["td"])[0]
    assert np.array_equal(same["log_probs"], c["logp"].reshape(T, ACT_W)) and same["approx_kl"] == 0 and (same["class"] == 0).all()


def test_rows_behind_the_batch_reach_nothing(case):
    c = case
    x = pm.stacks(c["obs"], S)[:T].reshape(T, S, OBS_W)
    args = (c["act"][:, 0], c["old"][:, 0], c["adv"][:, 0, 0], c["td"][:, 0, 0])
    want = um.agent_gradients(c["actor"], c["value"], x, *args, groups=2)
    pad = lambda v: np.concatenate([v, np.full((27,) + v.shape[1:], np.nan, dtype=F)])      # up to the end of the second tile
    got = um.agent_gradients(c["actor"], c["value"], pad(x), *[pad(v) for v in args], groups=2, live=T)
    for net in ("actor", "value"):
        assert all(np.array_equal(got[net][k], want[net][k]) for k in want[net]), net
    assert all(got[k] == want[k] for k in ("actor_loss", "critic_loss", "approx_kl"))


def test_the_stop_is_per_agent_and_begin_update_clears_it(case):
    c = case
    ep = epochs(c)
    args = (c["obs"], c["act"], c["old"], c["adv"], c["td"])
    kl = float(ep.gradients(*args)[0]["approx_kl"])
    ep.epoch_update(*args, kl_tolerance=abs(kl) * 10 + 1)       # 1.5 * tolerance is above approx_kl: no stop
    assert ep.flags == [0] and ep.steps == [1]
    kl2 = float(ep.gradients(*args)[0]["approx_kl"])
    tol = (kl2 - abs(kl2) * 0.5 - 1e-3) / 1.5                  # 1.5 * tol lies below this epoch's approx_kl
    ep.epoch_update(*args, kl_tolerance=tol)
    assert ep.flags == [1] and ep.steps == [2]                  # the flag is set BEHIND the step of the epoch that exceeds it
    snap = {k: v.copy() for k, v in ep.actor[0].items()}
    assert ep.epoch_update(*args) == [None] and ep.steps == [2]
    assert all(np.array_equal(ep.actor[0][k], snap[k]) for k in snap)
    ep.begin_update()
    ep.epoch_update(*args, kl_tolerance=float("inf"))
    assert ep.flags == [0] and ep.steps == [3] and not np.array_equal(ep.actor[0]["fc.weight"], snap["fc.weight"])


# ---------------------------------------------------------------------------------------------------- against the reference's update()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((4, 1, 4), (20, 4, 5), (56, 8, 5), (6, 2, 1))
SIZE_LIMIT = 666561


def load(case, name):
    with np.load(os.path.join(GOLDEN, f"ppoup_o{case[0]}_a{case[1]}_s{case[2]}_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def part(z, tag):
    return {k[len(tag) + 1:]: v for k, v in z.items() if k.startswith(tag + ".")}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "o%d_a%d_s%d" % c)
def test_the_model_meets_the_rule_against_the_references_update(case):
    """Per network, pooled over the recorded epochs: max_t(max|model_t - ref64_t| / max|ref64_t|) <= 4 max_t(max|ref32_t - ref64_t| /
    max|ref64_t|) over the clipped gradient tensors, and over the forward tensors with the single numbers (losses, approx_kl, norms);
    max|model - ref64| <= 4 max|ref32 - ref64| behind Adam for the parameters, exp_avg and exp_avg_sq of each network and epoch; the stop
    flag and the number of steps are the reference's."""
    obs_dim, act_dim, S = case
    inp = load(case, "in")
    info = json.loads(str(inp["info_json"]))
    assert (info["obs_dim"], info["act_dim"], info["stack_size"], info["T"]) == (obs_dim, act_dim, S, 37)
    for path in glob.glob(os.path.join(GOLDEN, "ppoup_o%d_a%d_s%d_*.npz" % case)):
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
        ep = um.Epochs(agents, [part(z["actor"], "p")], [part(z["value"], "p")], S)
        r = ep.gradients(*args, clip_eps=hyper["clip_eps"], max_grad_norm=hyper["max_grad_norm"])[0]
        fwd = [(r["log_probs"], z["actor"], "log_probs"), (r["values"], z["value"], "values"), (r["actor_loss"], z["actor"], "loss"),
               (r["critic_loss"], z["value"], "loss"), (r["approx_kl"], z["actor"], "approx_kl"), (r["actor_norm"], z["actor"], "norm"),
               (r["value_norm"], z["value"], "norm")]
        for mine, zz, key in fwd:
            ref32 = zz[key].astype(np.float64)
            ref64 = ref32 - zz["d" + key]
            if np.max(np.abs(ref64)) == 0:                      # epoch 0's approx_kl: every ratio is exactly 1, in the reference too
                assert np.all(np.asarray(mine) == 0) and np.all(ref32 == 0), key
                continue
            # (in epoch 0 approx_kl and actor_loss are sums that cancel to nearly nothing in float64 and exactly in float32: they decide the
            # pool of all epochs, so the epochs behind it are pooled once more by themselves)
            for name in ("forward",) + (("forward behind epoch 0",) if e else ()):
                worst[name][0] = max(worst[name][0], rel(np.asarray(mine).reshape(ref64.shape), ref64))
                worst[name][1] = max(worst[name][1], rel(ref32, ref64))
        assert F(r["actor_coef"]) == F(z["actor"]["coef"]) or abs(float(r["actor_coef"]) - float(z["actor"]["coef"])) <= 1e-5 * float(z["actor"]["coef"])
        for net, lr in (("actor", hyper["actor_lr"]), ("value", hyper["critic_lr"])):
            g32, dg = part(z[net], "g"), part(z[net], "dg")
            for key in g32:
                ref64 = g32[key].astype(np.float64) - dg[key]
                scale = np.max(np.abs(ref64))
                if scale == 0:
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
        ratios[k] = a / b
    print(case, {str(k): round(v, 2) for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v <= 4.0, (case, k, v)
    # the stop flag and the number of steps: the model's own chain from the first recorded parameters
    z0 = {net: load(case, f"e0_{net}_grad") for net in ("actor", "value")}
    ep = um.Epochs(agents, [part(z0["actor"], "p")], [part(z0["value"], "p")], S)
    ep.begin_update()
    for _ in range(info["epochs"]):
        ep.epoch_update(*args, **hyper)
    assert ep.steps == [info["epochs_run"]] and ep.flags == [int(info["stopped"])], (ep.steps, ep.flags, info["epochs_run"], info["stopped"])
