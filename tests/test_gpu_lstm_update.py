"""The recurrent PPO agents' clipped-loss epochs on the device (pednstream_amd/lstm.py: LstmPpoTargets.epoch_update, epoch_gradients,
update_store) against tests/lstm_update_model.py: bit for bit where the arithmetic is float32 (values, approx_kl,
critic_loss, the gates' gradients a[t], both gradient packs before and after clipping, norms, coefficients, parameters and Adam state, step
counts and flags), within section 20's 1-4 ulp allowances where libm in double is involved (std, log_probs, d_mu, d_z, actor_loss).  The
comparison is staged as tests/test_gpu_ppo_update.py's, whose checker this file uses: the kernel's own std, log_probs, d_mu and d_z are fed to
the model's next stage."""
import numpy as np
import pytest

import lstm_update_model as lum
from test_gpu_actors import host, same
from test_gpu_lstm import AGENTS, MAX_STD, MIN_STD, N_ACTIONS, N_OBS, make_env, random_sd
from test_gpu_ppo_update import HYPER, check_epoch, dev, padding_is_zero, staged

pytestmark = pytest.mark.gpu

F = np.float32
T_MAX, N_MAX = 97, 33
# one row; 65 rows that end a row tile in the middle of a step; two env tiles, the second of one env (99 rows, 4 row tiles: two groups take
# two each, three take 2, 1, 1); a single long sequence
SHAPES = ((1, 1, 2), (5, 13, 2), (3, 33, 2), (3, 33, 3), (97, 1, 3))

_setup = {}


def setup():
    """Parameters and a rollout: drawn once, shared, never written."""
    if not _setup:
        from pednstream_amd.lstm import actor_tensor_shapes, value_tensor_shapes

        rng = np.random.default_rng(2104)
        c = _setup
        c["actors"] = [random_sd(rng, actor_tensor_shapes(ow, aw)) for (_, ow, _, aw) in AGENTS]
        c["values"] = [random_sd(rng, value_tensor_shapes(ow)) for (_, ow, _, _) in AGENTS]
        c["obs"] = (rng.standard_normal((T_MAX + 1, N_MAX, N_OBS)) * 2 + 1).astype(F)
        c["actions"] = (rng.standard_normal((T_MAX, N_MAX, N_ACTIONS)) * 1.5).astype(F)
        c["adv"] = rng.standard_normal((T_MAX, N_MAX, len(AGENTS))).astype(F)
        c["td"] = rng.standard_normal((T_MAX, N_MAX, len(AGENTS))).astype(F)
        c["shift"] = (rng.standard_normal((T_MAX, N_MAX, N_ACTIONS)) * 0.25).astype(F)      # old_log_probs = evaluate's + shift: ratios around 1 +- 0.25
    return _setup


def make(min_std=MIN_STD, max_std=MAX_STD):
    pytest.importorskip("torch")
    from pednstream_amd.lstm import LstmActors, LstmPpoTargets

    c = setup()
    actors = LstmActors(AGENTS, np.zeros(N_ACTIONS, dtype=F), np.full(N_ACTIONS, 4.0, dtype=F), 1, N_OBS, N_ACTIONS, delta_actions=False,
                        min_std=min_std, max_std=max_std)
    ppo = LstmPpoTargets(actors)
    for i in range(len(AGENTS)):
        actors.load_state_dict(i, c["actors"][i])
        ppo.load_state_dict(i, c["values"][i])
    return ppo


def inputs(torch, ppo, c, T, N, envs=None):
    """The device tensors of the corner (T, N) of the rollout (or of the envs listed); old_log_probs are evaluate's on the loaded
    parameters, shifted."""
    e = slice(0, N) if envs is None else envs
    obs, act = dev(torch, c["obs"][:T + 1, e]), dev(torch, c["actions"][:T, e])
    old = ppo.evaluate(obs, act)["old_log_probs"] + dev(torch, c["shift"][:T, e])
    return obs, act, old.contiguous(), dev(torch, c["adv"][:T, e]), dev(torch, c["td"][:T, e])


def gate_gradients(ppo, T, N, groups):
    """a [2 (value, actor)][n_agents][T * N][256] as the backward left it in the activations"""
    return host(ppo._uout[(T, N, ppo._groups(groups))]["act"])[:, :, :, 128:]


def check_gates(ppo, res, T, N, groups, what):
    a = gate_gradients(ppo, T, N, groups)
    for i, r in enumerate(res):
        if r is not None:
            assert same(a[0, i], r["a_value"]), (what, "a of the value network", i, np.abs(a[0, i] - r["a_value"]).max())
            assert same(a[1, i], r["a_actor"]), (what, "a of the actor", i, np.abs(a[1, i] - r["a_actor"]).max())
            assert np.abs(r["a_actor"]).max() > 0 and np.abs(r["a_value"]).max() > 0


# ---------------------------------------------------------------------------------------------------- kernel == model
@pytest.mark.parametrize("T,N,groups", SHAPES)
def test_kernel_equals_the_model(T, N, groups):
    torch = pytest.importorskip("torch")
    c = setup()
    ppo = make()
    model = lum.Epochs(AGENTS, c["actors"], c["values"], MIN_STD, MAX_STD)
    args = inputs(torch, ppo, c, T, N)
    ah = dict(zip(("obs", "actions", "old", "adv", "td"), (host(a) for a in args)))
    what = (T, N, groups)
    # the gradients alone: nothing is stepped
    ppo.epoch_gradients(*args, groups=groups, want_tail=True)
    res = model.gradients(ah["obs"], ah["actions"], ah["old"], ah["adv"], ah["td"], groups=groups, stages=staged(ppo))
    check_epoch(ppo, model, res, ah, what + ("gradients",), stepped=False)
    check_gates(ppo, res, T, N, groups, what)
    for r in res:
        for net in ("actor", "value"):
            assert r[net]["lstm.bias_ih_l0"].tobytes() == r[net]["lstm.bias_hh_l0"].tobytes()
    assert ppo.adam_steps() == [0] * len(AGENTS) and not host(ppo.epoch_outputs.stop_flags).any()
    for i in range(len(AGENTS)):
        assert all(same(host(v), c["actors"][i][key]) for key, v in ppo.actors.parameters(i).items()), "epoch_gradients changed a parameter"
        assert all(same(host(v), c["values"][i][key]) for key, v in ppo.parameters(i).items()), "epoch_gradients changed a parameter"
    # one epoch and three
    for epoch in range(3):
        ppo.epoch_update(*args, groups=groups, want_tail=True, **HYPER)
        res = model.epoch_update(ah["obs"], ah["actions"], ah["old"], ah["adv"], ah["td"], groups=groups, stages=staged(ppo), **HYPER)
        check_epoch(ppo, model, res, ah, what + ("epoch", epoch), stepped=True)
        check_gates(ppo, res, T, N, groups, what + ("epoch", epoch))
    assert padding_is_zero(ppo), what
    assert float(host(ppo.epoch_outputs.actor_coef).max()) <= 1.0


def test_the_forward_is_evaluates_and_unit_ratios():
    torch = pytest.importorskip("torch")
    T, N = 5, 13
    c = setup()
    ppo = make()
    obs, act = dev(torch, c["obs"][:T + 1, :N]), dev(torch, c["actions"][:T, :N])
    ev = ppo.evaluate(obs, act)
    old, values = ev["old_log_probs"].clone(), host(ev["values"]).copy()
    ppo.epoch_gradients(obs, act, old, dev(torch, c["adv"][:T, :N]), dev(torch, c["td"][:T, :N]))
    o = ppo.epoch_outputs
    assert same(host(o.log_probs), host(old)) and same(host(o.values), values)
    assert (host(o.approx_kl) == 0).all()                       # every ratio is exp(0) = 1
    assert o.std is None and o.d_mu is None                     # (not asked for)


def test_a_row_depends_on_its_own_env_only():
    """env 12 of 13 gives the same log_probs, values and rows of a wherever it stands: moved to position 0 of a batch of 13 whose other envs
    differ, and alone (alone the number of rows differs, and with it the mean's weight in every gradient, so only the forward is compared)"""
    torch = pytest.importorskip("torch")
    T, N = 5, 13
    c = setup()
    ppo = make()
    args = inputs(torch, ppo, c, T, N)
    ppo.epoch_gradients(*args, groups=2, want_tail=True)
    o = ppo.epoch_outputs
    first = {k: host(getattr(o, k)).copy() for k in ("log_probs", "values", "d_mu")}
    a_first = gate_gradients(ppo, T, N, 2).reshape(2, len(AGENTS), T, N, 256).copy()
    moved = [12] + list(range(20, 32))                          # env 12 first, then twelve envs the first batch did not hold
    args2 = inputs(torch, ppo, c, T, N, envs=moved)
    ppo.epoch_gradients(*args2, groups=2, want_tail=True)
    o = ppo.epoch_outputs
    a_moved = gate_gradients(ppo, T, N, 2).reshape(2, len(AGENTS), T, N, 256)
    for k, v in first.items():
        assert same(host(getattr(o, k))[:, 0], v[:, 12]), k
        assert not same(host(getattr(o, k))[:, 1], v[:, 1]), k
    assert same(a_moved[:, :, :, 0], a_first[:, :, :, 12]) and np.abs(a_first[:, :, :, 12]).max() > 0
    alone = inputs(torch, ppo, c, T, 1, envs=[12])
    ppo.epoch_gradients(*alone, groups=2)
    o = ppo.epoch_outputs
    assert same(host(o.log_probs)[:, 0], first["log_probs"][:, 12]) and same(host(o.values)[:, 0], first["values"][:, 12])


# ---------------------------------------------------------------------------------------------------- the stop
def test_a_stopped_agent_is_left_alone_until_begin_update():
    torch = pytest.importorskip("torch")
    T, N = 5, 13
    c = setup()
    ppo = make()
    args = inputs(torch, ppo, c, T, N)
    model = lum.Epochs(AGENTS, c["actors"], c["values"], MIN_STD, MAX_STD)
    res = model.gradients(*[host(a) for a in args])
    kl = sorted(float(r["approx_kl"]) for r in res)
    assert kl[1] < kl[2] and (kl[2] - kl[1]) > 1e-4 * abs(kl[2]) and kl[2] > 0
    tol = 0.5 * (max(kl[1], 0.0) + kl[2]) / 1.5                 # 1.5 * tol lies between the two largest: exactly one agent stops
    stopper = [float(r["approx_kl"]) for r in res].index(kl[2])
    hyper = dict(HYPER, kl_tolerance=tol)
    ppo.epoch_update(*args, **hyper)
    assert host(ppo.epoch_outputs.stop_flags).tolist() == [int(i == stopper) for i in range(3)] and ppo.adam_steps() == [1, 1, 1]
    snap = lambda: ([host(v).copy() for v in ppo.actors.parameters(stopper).values()] + [host(v).copy() for v in ppo.parameters(stopper).values()] +
                    [host(v).copy() for d in ppo.adam_state(stopper, "actor") + ppo.adam_state(stopper, "value") for v in d.values()] +
                    [host(v).copy() for n in ("actor", "value") for v in ppo.epoch_outputs.grads(stopper, n).values()])
    other = (stopper + 1) % 3
    before, others = snap(), host(ppo.actors.parameters(other)["lstm.weight_hh_l0"]).copy()
    kl_before = host(ppo.epoch_outputs.approx_kl).copy()
    a0, aw = AGENTS[stopper][2], AGENTS[stopper][3]
    logp_before = host(ppo.epoch_outputs.log_probs)[:, :, a0:a0 + aw].copy()
    for _ in range(2):
        ppo.epoch_update(*args, **dict(hyper, kl_tolerance=float("inf")))
    assert all(same(a, b) for a, b in zip(snap(), before)), "a stopped agent changed"
    steps = ppo.adam_steps()
    assert steps[stopper] == 1 and all(s == 3 for i, s in enumerate(steps) if i != stopper)
    assert not same(host(ppo.actors.parameters(other)["lstm.weight_hh_l0"]), others)
    assert same(host(ppo.epoch_outputs.approx_kl)[stopper], kl_before[stopper])      # no output of it either
    assert same(host(ppo.epoch_outputs.log_probs)[:, :, a0:a0 + aw], logp_before)
    ppo.begin_update()
    assert not host(ppo.epoch_outputs.stop_flags).any()
    ppo.epoch_update(*args, **dict(hyper, kl_tolerance=float("inf")))
    assert ppo.adam_steps()[stopper] == 2 and not all(same(a, b) for a, b in zip(snap(), before))
    ppo.reset_adam()
    assert ppo.adam_steps() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------- bound modules, capture
def test_bound_modules_see_the_steps_and_agree_with_torch():
    """Three epochs on modules bound to the packs against the same three with torch autograd through the whole sequence and torch's Adam on
    unbound twins, compared as tests/test_gpu_ppo_update.py compares its step: the first epoch's gradients to rtol 1e-3 and 1e-5 of the
    tensor's largest, the parameters to 0.2 lr per step where the gradient is clear of rounding error.  The actions are samples of the
    policy, as a rollout's are."""
    torch = pytest.importorskip("torch")
    from pednstream_amd.lstm import make_actor_module, make_value_module

    T, N, lr = 5, 13, 3e-4
    c = setup()
    ppo = make()
    actors = ppo.actors
    obs, _, _, adv, td = inputs(torch, ppo, c, T, N)
    ev = ppo.evaluate(obs, torch.zeros(T, N, N_ACTIONS, device="cuda"), want_mu_std=True)
    act = (ev["mu"] + ev["std"] * dev(torch, np.random.default_rng(5).standard_normal((T, N, N_ACTIONS)).astype(F))).contiguous()
    old = (ppo.evaluate(obs, act)["old_log_probs"] + dev(torch, c["shift"][:T, :N])).contiguous()
    args = (obs, act, old, adv, td)
    amods, vmods, ref_a, ref_v = [], [], [], []
    for i, (_, ow, _, aw) in enumerate(AGENTS):
        a, v = make_actor_module(ow, aw, MIN_STD, MAX_STD).cuda(), make_value_module(ow).cuda()
        a.load_state_dict({k: torch.as_tensor(x) for k, x in c["actors"][i].items()})
        v.load_state_dict({k: torch.as_tensor(x) for k, x in c["values"][i].items()})
        ra, rv = make_actor_module(ow, aw, MIN_STD, MAX_STD).cuda(), make_value_module(ow).cuda()
        ra.load_state_dict(a.state_dict())
        rv.load_state_dict(v.state_dict())
        amods.append(actors.bind(i, a))
        vmods.append(ppo.bind(i, v))
        ref_a.append(ra)
        ref_v.append(rv)
        assert a.lstm.weight_hh_l0.data_ptr() == actors.parameters(i)["lstm.weight_hh_l0"].data_ptr()      # no copy: the module reads the pack
    first = {}
    seq = lambda v: v.transpose(0, 1)                                      # [T, N, ..] -> [N, T, ..]: a batch is an env
    for i, (o0, ow, a0, aw) in enumerate(AGENTS):
        x = seq(obs[:T, :, o0:o0 + ow]).contiguous()
        oa, ov = torch.optim.Adam(ref_a[i].parameters(), lr=lr), torch.optim.Adam(ref_v[i].parameters(), lr=lr)
        for epoch in range(3):
            mu, std, _ = ref_a[i](x)
            lp = torch.distributions.Normal(mu, std).log_prob(seq(act[:, :, a0:a0 + aw]))
            ratio = torch.exp((lp - seq(old[:, :, a0:a0 + aw])).clamp(-20, 20))
            A = seq(adv[:, :, i:i + 1])
            al = torch.mean(-torch.min(ratio * A, torch.clamp(ratio, 0.8, 1.2) * A))
            cl = torch.mean(torch.nn.functional.mse_loss(ref_v[i].forward_all_steps(x)[0], seq(td[:, :, i:i + 1])))
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
    before = host(amods[0].lstm.weight_hh_l0).copy()
    hyper = dict(HYPER, actor_lr=lr, critic_lr=lr)
    worst, moved, unclear = 0.0, 0.0, 0
    for epoch in range(3):
        ppo.epoch_update(*args, **hyper)
        if epoch == 0:
            for i in range(len(AGENTS)):
                for net, want in zip(("actor", "value"), first[i]):
                    got = ppo.epoch_outputs.grads(i, net)
                    for k, g in want.items():
                        assert torch.allclose(got[k], g, rtol=1e-3, atol=1e-5 * g.abs().max().item()), (i, net, k, (got[k] - g).abs().max().item())
    assert not same(host(amods[0].lstm.weight_hh_l0), before), "the bound module did not see the steps"
    with torch.no_grad():
        for i in range(len(AGENTS)):
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
    o0, ow, a0, aw = AGENTS[1]
    mu, _, _ = amods[1](seq(obs[:T, :, o0:o0 + ow]).contiguous())
    got = ppo.evaluate(obs, act, want_mu_std=True)["mu"][:, :, a0:a0 + aw]
    assert float((got - seq(mu)).abs().max()) <= 1e-4 * float(mu.abs().max())


def test_a_captured_update_store_gives_the_eager_bits():
    torch = pytest.importorskip("torch")
    from pednstream_amd.lstm import actor_tensor_shapes, value_tensor_shapes

    rows = 6
    env = make_env("nine_intersections", 4)
    actors = env.lstm_actors(seed=11)
    ppo = env.lstm_ppo_targets(actors)
    store = env.rollout_store(capacity=rows)
    rng = np.random.default_rng(12)
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        actors.load_state_dict(aid, random_sd(rng, actor_tensor_shapes(o.stop - o.start, a.stop - a.start), scale=1.0))
        ppo.load_state_dict(aid, random_sd(rng, value_tensor_shapes(o.stop - o.start), scale=1.0))
    roll = env.capture(lambda obs: actors.act(obs), on_step=lambda obs, rew: store.record(actors.outputs["raw"].double(), None))
    env.reset()
    store.begin()
    actors.reset_hidden()
    for _ in range(rows):
        roll.step()
    assert store.finish() == rows
    res = ppo.evaluate_store(store)
    old = res["old_log_probs"].clone()
    adv, td = ppo.compute_gae(store, res["values"], res["next_values"], 0.99, 0.95)
    adv = ((adv - adv.mean(dim=(0, 1))) / (adv.std(dim=(0, 1)) + 1e-8)).contiguous()      # the caller's normalisation line, per agent
    td = td.clone()
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
    allocated = torch.cuda.memory_allocated()
    ppo.update_store(store, old, adv, td, epochs=1, **hyper)             # nothing is allocated after the first call of a shape
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == allocated
    # the next evaluate_store reads the stepped packs
    assert not same(host(ppo.evaluate_store(store)["old_log_probs"]), host(old))
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
    store.close()
    env.close()


def test_refusals_on_device_tensors():
    torch = pytest.importorskip("torch")
    from pednstream_amd.lstm import LstmActors, LstmPpoTargets

    T, N = 3, 2
    c = setup()
    ppo = make()
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
    empty = LstmPpoTargets(LstmActors(AGENTS, np.zeros(N_ACTIONS, dtype=F), np.ones(N_ACTIONS, dtype=F), 1, N_OBS, N_ACTIONS, delta_actions=False))
    with pytest.raises(ValueError, match="no parameters were loaded"):
        empty.epoch_update(*args)
    for i in range(len(AGENTS)):
        empty.actors.load_state_dict(i, c["actors"][i])
    with pytest.raises(ValueError, match="no value networks"):
        empty.epoch_gradients(*args)
    assert ppo.adam_steps() == [0, 0, 0]
