"""PPO's clipped-loss epochs on the device (pednstream_amd/ppo.py: epoch_update, epoch_gradients, update_store) against
tests/ppo_update_model.py: bit for bit where the arithmetic is float32, within a few ulps where libm in double is involved.  The comparison is
staged as tests/test_gpu_sac_actor.py's: the kernel's own std, log_probs, d_mu and d_z are fed to the model's next stage, so that every
float32 stage is compared bit for bit whatever an ulp of libm did before it."""
import numpy as np
import pytest

import ppo_eval_model as pm
import ppo_update_model as um
from test_gpu_actors import host, random_sd, same
from test_gpu_ppo_eval import MAX_STD, MIN_STD, random_value
from test_gpu_sac_targets import TABLES, table, within_ulps

pytestmark = pytest.mark.gpu

F = np.float32
T_MAX, N_MAX = 97, 13
# 39 rows: a second tile of 7; one row; 97 rows = four tiles, two per group with groups = 2 and an uneven split with 3
SHAPES = ((3, 13, None), (1, 1, None), (97, 1, 2), (97, 1, 3))
HYPER = dict(actor_lr=3e-3, critic_lr=6e-3, clip_eps=0.2, max_grad_norm=0.5, kl_tolerance=float("inf"), betas=(0.9, 0.999), eps=1e-8)

_setups = {}


def setup(name, S):
    """Parameters and a rollout of a case: drawn once, shared, never written."""
    key = (name, S)
    if key not in _setups:
        agents, n_obs, n_actions = table(name)
        rng = np.random.default_rng(5000 * len(name) + 10 * S)
        actors = [random_sd(rng, "ppo", ow, aw, S) for (_, ow, _, aw) in agents]
        values = [random_value(rng, ow, S) for (_, ow, _, _) in agents]
        obs = (rng.standard_normal((T_MAX + 1, N_MAX, n_obs)) * 2 + 1).astype(F)
        actions = (rng.standard_normal((T_MAX, N_MAX, n_actions)) * 1.5).astype(F)
        adv = rng.standard_normal((T_MAX, N_MAX, len(agents))).astype(F)
        td = rng.standard_normal((T_MAX, N_MAX, len(agents))).astype(F)
        shift = (rng.standard_normal((T_MAX, N_MAX, n_actions)) * 0.25).astype(F)      # old_log_probs = evaluate's + shift: ratios around 1 +- 0.25
        _setups[key] = dict(agents=agents, n_obs=n_obs, n_actions=n_actions, actors=actors, values=values, obs=obs, actions=actions, adv=adv, td=td,
                            shift=shift)
    return _setups[key]


def make(name, S, min_std=MIN_STD, max_std=MAX_STD):
    pytest.importorskip("torch")
    from pednstream_amd.policy import StackedActors
    from pednstream_amd.ppo import PpoTargets

    c = setup(name, S)
    low, high = np.zeros(c["n_actions"], dtype=F), np.full(c["n_actions"], 4.0, dtype=F)
    actors = StackedActors("ppo", c["agents"], low, high, 1, c["n_obs"], c["n_actions"], stack_size=S, delta_actions=False, min_std=min_std,
                           max_std=max_std)
    ppo = PpoTargets(actors)
    for i in range(len(c["agents"])):
        actors.load_state_dict(i, c["actors"][i])
        ppo.load_state_dict(i, c["values"][i])
    return ppo


def dev(torch, v):
    return torch.as_tensor(np.ascontiguousarray(v)).cuda()


def inputs(torch, ppo, c, T, N):
    """The device tensors of the corner (T, N) of a case; old_log_probs are evaluate's on the loaded parameters, shifted."""
    obs, act = dev(torch, c["obs"][:T + 1, :N]), dev(torch, c["actions"][:T, :N])
    old = ppo.evaluate(obs, act)["old_log_probs"] + dev(torch, c["shift"][:T, :N])
    return obs, act, old.contiguous(), dev(torch, c["adv"][:T, :N]), dev(torch, c["td"][:T, :N])


def unpack(ppo, i, get):
    return {k: host(v) for k, v in get(i).items()}


def check_epoch(ppo, model, res, args_host, what, stepped):
    """One epoch's outputs against the model's result `res` (staged with the kernel's tail); with `stepped` the parameters and Adam state too."""
    o = ppo.epoch_outputs
    k = {n: host(getattr(o, n)) for n in ("log_probs", "values", "std", "d_mu", "d_z") + tuple(um_scalars())}
    flags = host(o.stop_flags)
    T, N = k["values"].shape[:2]
    for i, (o0, ow, a0, aw) in enumerate(model.agents):
        r = res[i]
        if r is None:
            continue
        sl = slice(a0, a0 + aw)
        flat = lambda v: v.reshape(T * N, -1)[:, sl]
        assert same(k["values"][:, :, i].reshape(-1), r["values"]), (what, "values", i)
        assert within_ulps(flat(k["std"]), r["own"]["std"], 1), (what, "std", i)
        assert within_ulps(flat(k["log_probs"]), pm.log_prob(flat(args_host["actions"]), r["mu"], flat(k["std"])), 2), (what, "log_probs", i)
        assert within_ulps(flat(k["d_mu"]), r["own"]["d_mu"], 4) and within_ulps(flat(k["d_z"]), r["own"]["d_z"], 4), (what, "tail", i)
        assert same(k["approx_kl"][i], r["approx_kl"]) and same(k["critic_loss"][i], r["critic_loss"]), (what, "approx_kl, critic_loss", i)
        assert abs(float(k["actor_loss"][i]) - float(r["actor_loss"])) <= 4 * float(np.spacing(np.abs(r["el"]).max())), (what, "actor_loss", i)
        for net in ("actor", "value"):
            raw, clipped = (unpack(ppo, i, lambda j: o.grads(model_id(ppo, j), net, clipped=c)) for c in (False, True))
            for key in r[net]:
                assert same(raw[key], r[net][key]), (what, net, "gradient", key, i, np.abs(raw[key] - r[net][key]).max())
                assert same(clipped[key], r[net + "_clipped"][key]), (what, net, "clipped gradient", key, i)
            assert same(k[net + "_norm"][i], r[net + "_norm"]) and same(k[net + "_coef"][i], r[net + "_coef"]), (what, net, "norm", i)
        if stepped:
            for net, params, get in (("actor", model.actor[i], ppo.actors.parameters), ("value", model.value[i], ppo.parameters)):
                now = unpack(ppo, i, lambda j: get(model_id(ppo, j)))
                m, v = ppo.adam_state(model_id(ppo, i), net)
                for key in params:
                    assert same(now[key], params[key]), (what, net, "parameter", key, i, np.abs(now[key] - params[key]).max())
                    assert same(host(m[key]), model.m[net][i][key]) and same(host(v[key]), model.v[net][i][key]), (what, net, "Adam state", key, i)
    if stepped:
        assert flags.tolist() == model.flags and ppo.adam_steps() == model.steps, (what, flags, model.flags, ppo.adam_steps(), model.steps)


def um_scalars():
    from pednstream_amd.ppo import SCALARS
    return SCALARS


def model_id(ppo, i):
    return ppo.agent_ids[i]


def staged(ppo):
    o = ppo.epoch_outputs
    return {"std": host(o.std), "logp": host(o.log_probs), "d_mu": host(o.d_mu), "d_z": host(o.d_z)}


def padding_is_zero(ppo):
    """the floats of the packs that belong to no tensor"""
    for pack, offsets in ((ppo.actors._device()["pack"], ppo.actors.offsets), (ppo._device()["pack"], ppo.offsets)):
        used = np.zeros(pack.numel(), dtype=bool)
        for off in offsets:
            for at, shape in off.values():
                used[at:at + int(np.prod(shape))] = True
        p = host(pack)
        if not (p[~used] == 0).all() or np.signbit(p[~used]).any():
            return False
    return True


# ---------------------------------------------------------------------------------------------------- kernel == model
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("name", list(TABLES))
def test_kernel_equals_the_model(name, S):
    torch = pytest.importorskip("torch")
    c = setup(name, S)
    for (T, N, groups) in SHAPES:
        ppo = make(name, S)
        model = um.Epochs(c["agents"], c["actors"], c["values"], S, MIN_STD, MAX_STD)
        args = inputs(torch, ppo, c, T, N)
        ah = dict(zip(("obs", "actions", "old", "adv", "td"), (host(a) for a in args)))
        what = (name, S, T, N, groups)
        # the gradients alone: nothing is stepped
        ppo.epoch_gradients(*args, groups=groups, want_tail=True)
        res = model.gradients(ah["obs"], ah["actions"], ah["old"], ah["adv"], ah["td"], groups=groups, stages=staged(ppo))
        check_epoch(ppo, model, res, ah, what + ("gradients",), stepped=False)
        assert ppo.adam_steps() == [0] * len(c["agents"]) and not host(ppo.epoch_outputs.stop_flags).any()
        for i in range(len(c["agents"])):
            assert all(same(host(v), c["actors"][i][key]) for key, v in ppo.actors.parameters(i).items()), "epoch_gradients changed a parameter"
        # one epoch and three
        for epoch in range(3):
            ppo.epoch_update(*args, groups=groups, want_tail=True, **HYPER)
            res = model.epoch_update(ah["obs"], ah["actions"], ah["old"], ah["adv"], ah["td"], groups=groups, stages=staged(ppo), **HYPER)
            check_epoch(ppo, model, res, ah, what + ("epoch", epoch), stepped=True)
        assert padding_is_zero(ppo), what
    # across the cases clip_grad_norm_ scales (random gradients of this size are far above 0.5)
    assert float(host(ppo.epoch_outputs.actor_coef).max()) <= 1.0


def test_the_forward_is_evaluates_and_unit_ratios():
    torch = pytest.importorskip("torch")
    name, S, T, N = "mixed", 5, 3, 13
    c = setup(name, S)
    ppo = make(name, S)
    obs, act = dev(torch, c["obs"][:T + 1, :N]), dev(torch, c["actions"][:T, :N])
    ev = ppo.evaluate(obs, act)
    old, values = ev["old_log_probs"].clone(), host(ev["values"])
    ppo.epoch_gradients(obs, act, old, dev(torch, c["adv"][:T, :N]), dev(torch, c["td"][:T, :N]))
    o = ppo.epoch_outputs
    assert same(host(o.log_probs), host(old)) and same(host(o.values), values[:T])
    assert (host(o.approx_kl) == 0).all()                       # every ratio is exp(0) = 1
    assert o.std is None and o.d_mu is None                     # (not asked for)
    # with every ratio 1 each element is a tie inside the range: actor_loss = mean(-A) over the agent's elements
    adv = c["adv"][:T, :N]
    for i, (_, _, _, aw) in enumerate(c["agents"]):
        el = np.repeat(-adv[:, :, i].reshape(-1, 1), aw, axis=1)
        want = um.reduce_groups([um.chain64(el[r0:r0 + 32]) for r0 in range(0, T * N, 32)], 512) / float(T * N * aw)
        assert same(host(o.actor_loss)[i], F(want)), i


def test_rows_behind_the_batch_and_awkward_values():
    torch = pytest.importorskip("torch")
    name, S, T, N = "mixed50", 5, 3, 13
    c = setup(name, S)
    ppo = make(name, S)
    args = inputs(torch, ppo, c, T, N)
    ppo.epoch_gradients(*args, groups=2, want_tail=True)
    first = {n: host(getattr(ppo.epoch_outputs, n)) for n in ("log_probs", "values", "actor_loss", "critic_loss", "actor_norm", "value_norm")}
    g_first = {k: host(v) for k, v in ppo.epoch_outputs.grads(1, "actor", clipped=False).items()}
    # obs row T is read by no stack of a row < T; slabs beyond G = 2 are read by nobody
    obs2 = args[0].clone()
    obs2[T] = float("nan")
    # the workspace need not be zeroed: a group STORES its first tile's partial, so NaN in every slab before the run reaches nothing
    ws = ppo._uout[(T, N, 2)]["ws"]
    assert ws.shape[0] == 2
    ws.fill_(float("nan"))
    ppo.epoch_gradients(obs2, *args[1:], groups=2, want_tail=True)
    for n, v in first.items():
        assert same(host(getattr(ppo.epoch_outputs, n)), v), n
    assert all(same(host(v), g_first[k]) for k, v in ppo.epoch_outputs.grads(1, "actor", clipped=False).items())
    # advantages == 0: no actor gradient at all, coefficient 1
    zero = torch.zeros_like(args[3])
    ppo.epoch_gradients(args[0], args[1], args[2], zero, args[4], groups=2)
    o = ppo.epoch_outputs
    assert (host(o.actor_norm) == 0).all() and (host(o.actor_coef) == 1).all() and (host(o.actor_loss) == 0).all()
    for i in range(len(c["agents"])):
        assert all((host(v) == 0).all() for v in o.grads(i, "actor").values())
    # a ratio exactly on 1 + clip_eps and on 1 - clip_eps: old = logp - log(bound) puts some there; the model decides which, the kernel agrees
    model = um.Epochs(c["agents"], c["actors"], c["values"], S, MIN_STD, MAX_STD)
    logp = ppo.evaluate(args[0], args[1])["old_log_probs"]
    old = logp.clone()
    old[0] = logp[0] - float(np.log(np.float64(F(1.2))))
    old[1] = logp[1] - float(np.log(np.float64(F(0.8))))
    ppo.epoch_gradients(args[0], args[1], old.contiguous(), args[3], args[4], groups=2, want_tail=True)
    ah = [host(a) for a in (args[0], args[1], old, args[3], args[4])]
    res = model.gradients(*ah, groups=2, stages=staged(ppo))
    check_epoch(ppo, model, res, {"actions": ah[1]}, "bounds", stepped=False)
    ratio = np.exp((host(ppo.epoch_outputs.log_probs) - ah[2]).astype(np.float64)).astype(F)
    assert (ratio[0] == F(1.2)).any() and (ratio[1] == F(0.8)).any(), "no ratio landed exactly on a bound"


def test_std_on_its_clamp_bounds():
    torch = pytest.importorskip("torch")
    name, S, T, N, lo, hi = "mixed", 5, 3, 13, 0.4, 1.2
    c = setup(name, S)
    ppo = make(name, S, min_std=lo, max_std=hi)
    model = um.Epochs(c["agents"], c["actors"], c["values"], S, lo, hi)
    args = inputs(torch, ppo, c, T, N)
    ppo.epoch_gradients(*args, want_tail=True)
    ah = [host(a) for a in args]
    res = model.gradients(*ah, stages=staged(ppo))
    std, d_z = host(ppo.epoch_outputs.std), host(ppo.epoch_outputs.d_z)
    assert (std == F(lo)).any() and (std == F(hi)).any() and ((std > F(lo)) & (std < F(hi))).any()
    own_sp_outside = np.concatenate([((r["own"]["std"] == F(lo)) | (r["own"]["std"] == F(hi))).reshape(-1) for r in res])
    assert own_sp_outside.any()
    check_epoch(ppo, model, res, {"actions": ah[1]}, "std bounds", stepped=False)
    assert (d_z[(std == F(lo)) | (std == F(hi))] == 0).all()     # (softplus lands exactly on a bound with probability nothing: blocked there)


# ---------------------------------------------------------------------------------------------------- the stop
def test_the_stop_is_per_agent():
    torch = pytest.importorskip("torch")
    from pednstream_amd.policy import StackedActors
    from pednstream_amd.ppo import PpoTargets

    # nine_intersections' three agents' shapes: 15, 20 and 15 observation columns, 3, 4 and 3 actions
    agents = [(0, 15, 0, 3), (15, 20, 3, 4), (35, 15, 7, 3)]
    S, T, N = 5, 3, 13
    rng = np.random.default_rng(77)
    actors_sd = [random_sd(rng, "ppo", ow, aw, S) for (_, ow, _, aw) in agents]
    values_sd = [random_value(rng, ow, S) for (_, ow, _, _) in agents]
    sa = StackedActors("ppo", agents, np.zeros(10, dtype=F), np.full(10, 4.0, dtype=F), 1, 50, 10, stack_size=S, delta_actions=False)
    ppo = PpoTargets(sa)
    for i in range(3):
        sa.load_state_dict(i, actors_sd[i])
        ppo.load_state_dict(i, values_sd[i])
    obs = dev(torch, (rng.standard_normal((T + 1, N, 50)) * 2 + 1).astype(F))
    act = dev(torch, (rng.standard_normal((T, N, 10)) * 1.5).astype(F))
    old = ppo.evaluate(obs, act)["old_log_probs"] + dev(torch, (rng.standard_normal((T, N, 10)) * 0.25).astype(F))
    adv, td = dev(torch, rng.standard_normal((T, N, 3)).astype(F)), dev(torch, rng.standard_normal((T, N, 3)).astype(F))
    args = (obs, act, old.contiguous(), adv, td)
    model = um.Epochs(agents, actors_sd, values_sd, S)
    res = model.gradients(*[host(a) for a in args])
    kl = sorted(float(r["approx_kl"]) for r in res)
    assert kl[1] < kl[2] and (kl[2] - kl[1]) > 1e-4 * abs(kl[2])
    tol = 0.5 * (kl[1] + kl[2]) / 1.5                           # 1.5 * tol lies between the two largest: exactly one agent stops
    stopper = [float(r["approx_kl"]) for r in res].index(kl[2])
    hyper = dict(HYPER, kl_tolerance=tol)
    ppo.epoch_update(*args, **hyper)
    assert host(ppo.epoch_outputs.stop_flags).tolist() == [int(i == stopper) for i in range(3)] and ppo.adam_steps() == [1, 1, 1]
    snap = lambda: ([host(v).copy() for v in sa.parameters(stopper).values()] + [host(v).copy() for v in ppo.parameters(stopper).values()] +
                    [host(v).copy() for d in ppo.adam_state(stopper, "actor") + ppo.adam_state(stopper, "value") for v in d.values()])
    before, others = snap(), host(sa.parameters((stopper + 1) % 3)["fc.weight"]).copy()
    kl_before = host(ppo.epoch_outputs.approx_kl).copy()
    for _ in range(2):
        ppo.epoch_update(*args, **dict(hyper, kl_tolerance=float("inf")))
    assert all(same(a, b) for a, b in zip(snap(), before)), "a stopped agent changed"
    steps = ppo.adam_steps()
    assert steps[stopper] == 1 and all(s == 3 for i, s in enumerate(steps) if i != stopper)
    assert not same(host(sa.parameters((stopper + 1) % 3)["fc.weight"]), others)
    assert same(host(ppo.epoch_outputs.approx_kl)[stopper], kl_before[stopper])      # no output of it either
    ppo.begin_update()
    assert not host(ppo.epoch_outputs.stop_flags).any()
    ppo.epoch_update(*args, **dict(hyper, kl_tolerance=float("inf")))
    assert ppo.adam_steps()[stopper] == 2 and not all(same(a, b) for a, b in zip(snap(), before))
    ppo.reset_adam()
    assert ppo.adam_steps() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------- bound modules, capture, refusals
def test_bound_modules_see_the_steps_and_agree_with_torch():
    """Three epochs on modules bound to the packs against the same three in torch (the epochs of examples/ppo_update.py, torch's Adam) on
    unbound twins, compared as tests/test_gpu_sac_critic.py compares its step: the first epoch's gradients to rtol 1e-3 and 1e-5 of the
    tensor's largest, the parameters to 0.2 lr per step where the gradient is clear of rounding error (Adam moves an element whose
    gradient is all rounding error by lr along the error's sign).  The actions are samples of the policy, as a rollout's are: far from mu
    the log-probabilities run into the hundreds and float32 torch itself is 3e-4 from a float64 twin."""
    torch = pytest.importorskip("torch")
    from pednstream_amd.policy import make_module
    from pednstream_amd.ppo import make_value_module

    name, S, T, N, lr = "mixed50", 5, 3, 13, 3e-4
    c = setup(name, S)
    ppo = make(name, S)
    actors = ppo.actors
    obs, _, _, adv, td = inputs(torch, ppo, c, T, N)
    ev = ppo.evaluate(obs, torch.zeros(T, N, c["n_actions"], device="cuda"), want_mu_std=True)
    act = (ev["mu"] + ev["std"] * dev(torch, np.random.default_rng(5).standard_normal((T, N, c["n_actions"])).astype(F))).contiguous()
    old = (ppo.evaluate(obs, act)["old_log_probs"] + dev(torch, c["shift"][:T, :N])).contiguous()
    args = (obs, act, old, adv, td)
    amods, vmods, ref_a, ref_v = [], [], [], []
    for i, (_, ow, _, aw) in enumerate(c["agents"]):
        a, v = make_module("ppo", ow, aw, S, MIN_STD, MAX_STD).cuda(), make_value_module(ow, S).cuda()
        a.load_state_dict({k: torch.as_tensor(x) for k, x in c["actors"][i].items()})
        v.load_state_dict({k: torch.as_tensor(x) for k, x in c["values"][i].items()})
        ra, rv = make_module("ppo", ow, aw, S, MIN_STD, MAX_STD).cuda(), make_value_module(ow, S).cuda()
        ra.load_state_dict(a.state_dict())
        rv.load_state_dict(v.state_dict())
        amods.append(actors.bind(i, a))
        vmods.append(ppo.bind(i, v))
        ref_a.append(ra)
        ref_v.append(rv)
        assert a.fc.weight.data_ptr() == actors.parameters(i)["fc.weight"].data_ptr()      # no copy: the module reads the pack
    t_idx = torch.as_tensor(pm.stack_times(T, S)[:T]).cuda()
    stacks = obs[t_idx].transpose(1, 2).reshape(T * N, S, -1)
    first = {}
    for i, (o0, ow, a0, aw) in enumerate(c["agents"]):
        x = stacks[:, :, o0:o0 + ow].contiguous()
        oa, ov = torch.optim.Adam(ref_a[i].parameters(), lr=lr), torch.optim.Adam(ref_v[i].parameters(), lr=lr)
        for epoch in range(3):
            mu, std = ref_a[i](x)
            lp = torch.distributions.Normal(mu, std).log_prob(act.reshape(T * N, -1)[:, a0:a0 + aw])
            ratio = torch.exp((lp - old.reshape(T * N, -1)[:, a0:a0 + aw]).clamp(-20, 20))
            A = adv.reshape(T * N, -1)[:, i:i + 1]
            al = torch.mean(-torch.min(ratio * A, torch.clamp(ratio, 0.8, 1.2) * A))
            cl = torch.mean(torch.nn.functional.mse_loss(ref_v[i](x), td.reshape(T * N, -1)[:, i:i + 1]))
            oa.zero_grad()
            ov.zero_grad()
            al.backward()
            cl.backward()
            torch.nn.utils.clip_grad_norm_(ref_a[i].parameters(), 0.5)
            torch.nn.utils.clip_grad_norm_(ref_v[i].parameters(), 0.5)
            if epoch == 0:
                first[i] = [{k: p.grad.clone() for k, p in m.named_parameters()} for m in (ref_a[i], ref_v[i])]
            oa.step()
            ov.step()
    before = host(amods[0].fc.weight).copy()
    hyper = dict(HYPER, actor_lr=lr, critic_lr=lr)
    worst, moved, unclear = 0.0, 0.0, 0
    for epoch in range(3):
        ppo.epoch_update(*args, **hyper)
        if epoch == 0:
            for i in range(len(c["agents"])):
                for net, want in zip(("actor", "value"), first[i]):
                    got = ppo.epoch_outputs.grads(i, net)
                    for k, g in want.items():
                        assert torch.allclose(got[k], g, rtol=1e-3, atol=1e-5 * g.abs().max().item()), (i, net, k)
    assert not same(host(amods[0].fc.weight), before), "the bound module did not see the steps"
    with torch.no_grad():
        for i in range(len(c["agents"])):
            for mods, refs, want, sds in ((amods, ref_a, first[i][0], c["actors"]), (vmods, ref_v, first[i][1], c["values"])):
                for (k, p), (_, q) in zip(mods[i].named_parameters(), refs[i].named_parameters()):
                    clear = want[k].abs() > 1e-4 * want[k].abs().max()
                    unclear += int((~clear).sum())
                    assert clear.any() and torch.allclose(p[clear], q[clear], rtol=0, atol=3 * 0.2 * lr), (i, k, (p - q)[clear].abs().max().item())
                    worst = max(worst, float((p - q)[clear].abs().max()))
                    moved = max(moved, float(np.abs(host(p) - sds[i][k]).max()))
    print(f"device vs torch behind three epochs: max |difference| {worst:.3g} in parameters the steps moved by {moved:.3g} ({unclear} elements left out)")
    assert moved > 2 * lr
    # evaluate reads the stepped packs: its mu is the bound module's
    o0, ow, a0, aw = c["agents"][1]
    mu, _ = amods[1](stacks[:, :, o0:o0 + ow].contiguous())
    got = ppo.evaluate(obs, act, want_mu_std=True)["mu"].reshape(T * N, -1)[:, a0:a0 + aw]
    assert float((got - mu).abs().max()) <= 1e-4 * float(mu.abs().max())


def test_a_captured_update_store_gives_the_eager_bits():
    torch = pytest.importorskip("torch")
    from test_gpu_actors import env_actors, nine

    S, rows = 4, 6
    env = nine(4)
    buf = env.replay_store(rows + 2, stack_size=S, seed=1)
    actors, _ = env_actors(env, "ppo", S)
    store = env.rollout_store(capacity=rows)
    ppo = env.ppo_targets(actors)
    rng = np.random.default_rng(12)
    for aid in env.possible_agents:
        o = env.obs_slices[aid]
        ppo.load_state_dict(aid, random_value(rng, o.stop - o.start, S, scale=1.0))
    roll = env.capture(lambda obs: actors.act(buf.stacked_obs()),
                       on_step=lambda obs, rew: (buf.push(actors.actions), store.record(actors.outputs["raw"].double(), None)))
    env.reset()
    buf.begin()
    store.begin()
    for _ in range(rows):
        roll.step()
    assert store.finish() == rows
    old = ppo.evaluate_store(store).clone()
    adv, td = store.compute_gae(0.99, 0.95, normalize=True)
    torch.cuda.synchronize()
    hyper = dict(HYPER, actor_lr=1e-2, critic_lr=1e-2, kl_tolerance=0.01)
    packs_ = (actors._device()["pack"], ppo._device()["pack"])
    start = [p.clone() for p in packs_]
    state = lambda: [host(p).copy() for p in packs_] + [host(ppo._update_device()[n][k]).copy() for n in ("actor", "value") for k in ("exp_avg", "exp_avg_sq")] \
        + [np.array(ppo.adam_steps()), host(ppo._update_device()["flags"]).copy()]

    def restore():
        for p, s in zip(packs_, start):
            p.copy_(s)
        ppo.reset_adam()

    ppo.update_store(store, old, adv, td, epochs=3, **hyper)             # eager (allocates the workspace and the outputs)
    torch.cuda.synchronize()
    eager = state()
    assert not same(eager[0], host(start[0])) and max(ppo.adam_steps()) >= 1
    # the next evaluate_store reads the stepped packs
    assert not same(host(ppo.evaluate_store(store)), host(old))
    restore()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                               # one stream: a single chain of launches
        ppo.update_store(store, old, adv, td, epochs=3, **hyper)
    for replay in range(2):
        restore()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        now = state()
        names = ("actor pack", "value pack", "actor exp_avg", "actor exp_avg_sq", "value exp_avg", "value exp_avg_sq", "steps", "flags")
        differ = [n for n, a, b in zip(names, now, eager) if not same(a, b)]
        assert not differ, ("a replay differs from the eager run", replay, differ, now[6:], eager[6:])
    with pytest.raises(ValueError, match="epochs"):
        ppo.update_store(store, old, adv, td, epochs=-1)
    buf.close()
    store.close()
    env.close()


def test_refusals_on_device_tensors():
    torch = pytest.importorskip("torch")
    name, S, T, N = "one", 1, 3, 2
    c = setup(name, S)
    ppo = make(name, S)
    args = list(inputs(torch, ppo, c, T, N))
    for i, nm in enumerate(("obs", "actions", "old_log_probs", "advantages", "td_target")):
        bad = list(args)
        bad[i] = args[i][:, :1].contiguous() if i else args[i][:, :, :0]
        with pytest.raises(ValueError, match=nm if i else "obs|n_obs"):
            ppo.epoch_update(*bad)
        if nm != "actions":
            bad[i] = args[i].double()
            with pytest.raises(ValueError, match=nm):
                ppo.epoch_update(*bad)
        bad[i] = args[i].transpose(0, 1)
        with pytest.raises(ValueError):
            ppo.epoch_update(*bad)
    from pednstream_amd.policy import StackedActors
    from pednstream_amd.ppo import PpoTargets

    empty = PpoTargets(StackedActors("ppo", c["agents"], np.zeros(1, dtype=F), np.ones(1, dtype=F), 1, c["n_obs"], c["n_actions"], stack_size=S,
                                     delta_actions=False))
    with pytest.raises(ValueError, match="no actor parameters"):
        empty.epoch_update(*args)
    empty.actors.load_state_dict(0, c["actors"][0])
    with pytest.raises(ValueError, match="no value networks"):
        empty.epoch_gradients(*args)
    assert ppo.adam_steps() == [0]
