"""The SAC actor and temperature step on the device (pednstream_amd/sac.py: actor_update, actor_gradients;
pednstream_amd/csrc/pedn_actor_grad.hpp) against the contract's numpy restatement (tests/sac_actor_model.py): plain tensors, bound torch
modules, a captured whole update and an env's store.  The checks are staged like test_gpu_sac_critic's: what the contract evaluates in
float32 is compared bit for bit, what it evaluates in float64 and rounds once (the two tails, Adam's step scalars) within 2 ulps, and every
later stage is fed the kernel's own earlier outputs.  The tables and the minibatches are test_gpu_sac_targets': its next states serve as
states."""
import numpy as np
import pytest

import actor_model as am
import sac_actor_model as mm
import sac_critic_model as cm
import sac_target_model as sm
from test_gpu_actors import host, nine, same
from test_gpu_sac_targets import MAX_DELTA, N_MAX, TABLES, make, random_critic, setup, within_ulps

pytestmark = pytest.mark.gpu

TILE = 32
BATCHES = (1, 3, TILE + 1, 130)       # one row, less than a tile, a tile and a row, many tiles with a ragged last one
F = np.float32
STAGED = ("mu", "z", "std", "eps", "t", "new_actions", "logp", "d_mu", "d_z")


def unpack(offsets, flat):
    """[agent] = {key: array} of a host copy of an actors' pack"""
    return [{k: flat[at:at + int(np.prod(shape))].reshape(shape) for k, (at, shape) in cur.items()} for cur in offsets]


def unpack_critics(sac, flat):
    return [[{k: flat[at:at + int(np.prod(shape))].reshape(shape) for k, (at, shape) in cur.items()} for cur in pair] for pair in sac.offsets]


def padding(sac):
    pad = np.ones(sac.actors.pack_size, dtype=bool)
    for cur in sac.actors.offsets:
        for at, shape in cur.values():
            pad[at:at + int(np.prod(shape))] = False
    return pad


def snapshot(sac):
    d, ad = sac._device(), sac._actor_device()
    out = {"actor": host(sac.actors._device()["pack"]), "online": host(d["online"]), "target": host(d["target"]), "log_alpha": host(d["log_alpha"]),
           "exp_avg": host(ad["exp_avg"]), "exp_avg_sq": host(ad["exp_avg_sq"]), "alpha_moments": host(ad["alpha_moments"]), "adam": host(ad["adam"]),
           "grads": host(ad["grads"]), "scalars": host(ad["scalars"])}
    return {k: v.copy() for k, v in out.items()}


def outputs(sac):
    o = sac.actor_outputs
    return {k: host(getattr(o, k)).copy() for k in STAGED + ("entropy", "q1", "q2", "actor_loss", "alpha_loss", "alpha_grad")}


def check_forward_and_gradients(sac, agents, before, s, tent, what="", want_eps=None):
    """Every output of the last launch and its gradient pack against the model on the state `before` (a snapshot), staged."""
    out = outputs(sac)
    B = s.shape[0]
    actors, critics = unpack(sac.actors.offsets, before["actor"]), unpack_critics(sac, before["online"])
    grads = unpack(sac.actors.offsets, host(sac._actor_device()["grads"]))
    assert out["mu"].shape == (B, sac.n_actions) and out["q1"].shape == (B, len(agents)) and out["actor_loss"].shape == (len(agents),)
    if want_eps is not None:
        assert same(out["eps"], want_eps), (what, "eps")
    for i, (o0, ow, a0, aw) in enumerate(agents):
        sl, x = slice(a0, a0 + aw), s[:, :, o0:o0 + ow]
        c1, c2 = critics[i]
        k = {name: out[name][:, sl] for name in STAGED}
        k.update(entropy=out["entropy"][:, i], q1=out["q1"][:, i], q2=out["q2"][:, i])
        mu, z, std = am.forward("sac", actors[i], x)
        assert same(k["mu"], mu) and same(k["z"], z), (what, "mu, z", i)
        assert within_ulps(k["std"], std, 1), (what, "std", i)
        u, t, na, logp = sm.tail(k["mu"], k["std"], k["eps"], MAX_DELTA)
        assert within_ulps(k["t"], t, 2) and within_ulps(k["new_actions"], na, 2), (what, "t, new_actions", i)
        assert within_ulps(k["logp"], sm.log_prob(u, k["mu"], k["std"], k["t"]), 2), (what, "logp", i)
        assert same(k["entropy"], sm.entropy(k["logp"])), (what, "entropy", i)
        assert same(k["q1"], sm.critic(c1, x, k["new_actions"])) and same(k["q2"], sm.critic(c2, x, k["new_actions"])), (what, "q", i)
        d_mu, d_z = mm.head_gradients(k, mm.dq_daction(c1, aw), mm.dq_daction(c2, aw), before["log_alpha"][i], B, MAX_DELTA)
        assert within_ulps(k["d_mu"], d_mu, 2) and within_ulps(k["d_z"], d_z, 2), (what, "head gradients", i, np.abs(k["d_mu"] - d_mu).max())
        g, sc, _ = mm.gradients(actors[i], c1, c2, x, k["eps"], before["log_alpha"][i], tent[i], MAX_DELTA, stages=k)
        for name in ("actor_loss", "alpha_loss", "alpha_grad"):
            assert same(out[name][i], sc[name]), (what, name, i, out[name][i], sc[name])
        for key in g:
            assert same(grads[i][key], g[key]), (what, "gradient", i, key, np.abs(grads[i][key] - g[key]).max())
        views = sac.actor_outputs.grads(sac.agent_ids[i])
        assert list(views) == list(actors[i]) and all(same(host(views[key]), grads[i][key]) for key in g)
    return out


def check_adam(sac, before, t, hyper, what=""):
    """The moments (bit for bit) and the parameters (2 ulps: the step scalars) of the actors and of log_alpha behind step t, against the
    model on the state `before` and the launch's own gradients; the padding stays +0.0; nothing of the critics is written."""
    now = snapshot(sac)
    kw = dict(betas=hyper["betas"], eps=hyper["eps"])
    p, m, v = mm.adam(before["actor"], now["grads"], before["exp_avg"], before["exp_avg_sq"], t, lr=hyper["actor_lr"], **kw)
    differ = np.flatnonzero(now["exp_avg_sq"].view(np.uint32) != v.view(np.uint32))
    assert same(now["exp_avg"], m) and same(now["exp_avg_sq"], v), (what, "the actors' moments", t, differ.size, now["exp_avg_sq"][differ[:4]], v[differ[:4]])
    assert within_ulps(now["actor"], p, 2), (what, "the actors' parameters", t, np.abs(now["actor"] - p).max())
    p, m, v = mm.adam(before["log_alpha"], now["scalars"][2], before["alpha_moments"][0], before["alpha_moments"][1], t, lr=hyper["alpha_lr"], **kw)
    assert same(now["alpha_moments"][0], m) and same(now["alpha_moments"][1], v), (what, "log_alpha's moments", t)
    assert within_ulps(now["log_alpha"], p, 2) and not same(now["log_alpha"], before["log_alpha"]), (what, "log_alpha", t)
    assert same(now["online"], before["online"]) and same(now["target"], before["target"]), (what, "a critic pack was written")
    assert now["adam"][0] == t and now["adam"][1] == 0
    want = [1.0, 1.0]
    for _ in range(t):
        want = [want[0] * hyper["betas"][0], want[1] * hyper["betas"][1]]
    assert now["adam"][2:].view(np.float64).tolist() == want      # the running products, in double
    pad = padding(sac)
    for k in ("actor", "grads", "exp_avg", "exp_avg_sq"):
        assert not now[k][:pad.size][pad].view(np.uint32).any(), (what, "padding", k)
    return now


def restore(torch, sac, start):
    sac.actors._device()["pack"].copy_(torch.as_tensor(start["actor"]))
    sac.log_alpha.copy_(torch.as_tensor(start["log_alpha"]))
    sac.reset_actor_adam()


# ---------------------------------------------------------------------------------------------------- plain tensors
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("name", list(TABLES))
def test_kernel_equals_the_model(name, S):
    torch = pytest.importorskip("torch")
    c = setup(name, S)
    agents = c["agents"]
    sac = make(name, S)
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()
    hyper = dict(actor_lr=1e-2, alpha_lr=2e-2, betas=(0.9, 0.999), eps=1e-8)      # (steps large enough to move every parameter by many ulps)
    tent = [-0.5 * aw - 0.25 * i for i, (_, _, _, aw) in enumerate(agents)]
    assert name != "mixed" or padding(sac).any()
    start = snapshot(sac)
    whole = None
    for B in reversed(BATCHES):
        s, nz = c["ns"][:B], c["noise"][:B]
        ds, dn = dev(s), dev(nz)
        # the launches with the Adam steps switched off write nothing but their outputs
        sac.actor_gradients(ds, dn, target_entropy=tent)
        after = snapshot(sac)
        for k in ("actor", "online", "target", "log_alpha", "exp_avg", "exp_avg_sq", "alpha_moments", "adam"):
            assert same(after[k], start[k]), (B, k)
        out = check_forward_and_gradients(sac, agents, start, s, tent, what=("gradients", B), want_eps=nz)
        if B == N_MAX:
            whole = out
            lower = out["q2"] < out["q1"]
            assert lower.any() and not lower.all()                 # the minimum switches between the critics
        else:                                                      # a row's forward does not depend on the batch
            for k in STAGED[:7] + ("entropy", "q1", "q2"):
                assert same(out[k], whole[k][:B]), (B, k)
        # three updates, each checked from the state the launch found
        before = after
        for t in (1, 2, 3):
            sac.actor_update(ds, dn, target_entropy=tent, **hyper)
            if t == 1:
                assert same(host(sac._actor_device()["grads"]), after["grads"]), B      # the same gradients with the steps switched on
            else:
                check_forward_and_gradients(sac, agents, before, s, tent, what=("update", B, t))
            before = check_adam(sac, before, t, hyper, what=B)
        assert sac.actor_adam_steps() == 3 and not same(before["actor"], start["actor"]) and sac.actor_draws() == 0
        again = sac.actor_outputs
        sac.actor_gradients(ds, dn, target_entropy=tent)
        assert again.mu.data_ptr() == sac.actor_outputs.mu.data_ptr()      # allocated once per batch size
        restore(torch, sac, start)                                 # back to the start for the next batch size
        assert sac.actor_adam_steps() == 0
        for k, v in snapshot(sac).items():
            if k not in ("grads", "scalars"):
                assert same(v, start[k]), k
    # row position: row 77 of the 130-row launch alone, as row 0 of a launch of one
    sac.actor_gradients(dev(c["ns"][77:78]), dev(c["noise"][77:78]), target_entropy=tent)
    out = outputs(sac)
    for k in STAGED[:7] + ("entropy", "q1", "q2"):
        assert same(out[k], whole[k][77:78]), k


def test_the_forward_is_td_targets_and_critic_gradients():
    """mu and std are the bits td_target gives for the same rows and noise; q1 and q2 are the bits critic_gradients gives when the stored
    actions are new_actions."""
    torch = pytest.importorskip("torch")
    name, S, B = "mixed50", 5, 70
    c = setup(name, S)
    sac = make(name, S)
    s, nz, r, d = (torch.as_tensor(c[k][:B]).cuda() for k in ("ns", "noise", "rewards", "dones"))
    sac.actor_gradients(s, nz)
    out = sac.actor_outputs
    td = sac.td_target(r, s, d, noise=nz)
    for k in ("mu", "std", "eps", "logp", "entropy"):
        assert same(host(getattr(out, k)), host(sac.outputs[k])), k
    assert same(host(out.new_actions), host(sac.outputs["next_actions"]))
    sac.critic_gradients(s, out.new_actions, td)
    assert same(host(out.q1), host(sac.critic_outputs.q1)) and same(host(out.q2), host(sac.critic_outputs.q2))


def test_rows_behind_the_batch_and_awkward_values():
    """A ragged last tile reads nothing behind the batch: the tensors of a 33-row launch are views of larger ones whose later rows are
    NaN and inf.  A NaN inside the batch reaches the sums of its agent and of no other."""
    torch = pytest.importorskip("torch")
    name, S, B = "mixed", 5, TILE + 1
    c = setup(name, S)
    sac = make(name, S)
    start = snapshot(sac)
    tent = [-float(aw) for (_, _, _, aw) in c["agents"]]
    s, nz = (torch.as_tensor(c[k][:B + 40].copy()).cuda() for k in ("ns", "noise"))
    s[B:], nz[B:] = float("nan"), float("inf")
    sac.actor_gradients(s[:B], nz[:B])
    check_forward_and_gradients(sac, c["agents"], start, c["ns"][:B], tent)
    clean = snapshot(sac)
    assert np.isfinite(clean["grads"]).all() and np.isfinite(clean["scalars"]).all()
    o0 = c["agents"][1][0]
    s[B - 1, 2, o0 + 3] = float("nan")                        # one column of agent 1, in the last row
    sac.actor_gradients(s[:B], nz[:B])
    now = snapshot(sac)
    got, was = unpack(sac.actors.offsets, now["grads"]), unpack(sac.actors.offsets, clean["grads"])
    assert np.isnan(now["scalars"][:, 1]).all() and np.isfinite(now["scalars"][:, [0, 2]]).all()
    for i in (0, 2):
        assert all(same(got[i][k], was[i][k]) for k in got[i])
    assert np.isnan(got[1]["fc_mu.bias"]).all()
    check_forward_and_gradients(sac, c["agents"], start, host(s[:B]), tent)


# ---------------------------------------------------------------------------------------------------- bound modules
def test_bound_modules_see_the_steps_and_act_reads_them():
    torch = pytest.importorskip("torch")
    from pednstream_amd.policy import make_module
    from pednstream_amd.sac import WHICH, make_critic_module

    name, S, B, steps, lr = "mixed50", 5, 40, 3, 1e-2
    c = setup(name, S)
    agents = c["agents"]
    sac = make(name, S)
    torch.manual_seed(4)
    s, nz = (torch.as_tensor(c[k][:B]).cuda() for k in ("ns", "noise"))
    mods, twins, leaves, twin_leaves = [], [], [], []
    for i, (o0, ow, a0, aw) in enumerate(agents):
        actor = make_module("sac", ow, aw, S).cuda()
        with torch.no_grad():
            actor.fc_std.bias.add_(0.5)
        four = [make_critic_module(ow, aw, S).cuda() for _ in WHICH]
        with torch.no_grad():
            for p in four[1].parameters():
                p.mul_(1.3)
        leaf = torch.tensor(float(c["log_alpha"][i]), device="cuda", requires_grad=True)
        twin = make_module("sac", ow, aw, S).cuda()
        twin.load_state_dict({k: v.clone() for k, v in actor.state_dict().items()})
        twin_leaves.append(leaf.detach().clone().requires_grad_(True))
        sac.actors.bind(i, actor)
        sac.bind(i, *four, log_alpha=leaf)
        mods.append((actor, four))
        twins.append(twin)
        leaves.append(leaf)
    start = snapshot(sac)
    # the reference's actor half on copies, with torch.optim.Adam: the same steps up to the order of the sums
    opt = torch.optim.Adam([p for m in twins for p in m.parameters()], lr=lr)
    opt_alpha = torch.optim.Adam(twin_leaves, lr=lr)
    for _ in range(steps):
        sac.actor_update(s, nz, actor_lr=lr, alpha_lr=lr)
        opt.zero_grad()
        opt_alpha.zero_grad()
        for i, (o0, ow, a0, aw) in enumerate(agents):
            x = s[:, :, o0:o0 + ow]
            mu, std = twins[i](x)
            u = mu + std * nz[:, a0:a0 + aw]
            logp = torch.distributions.Normal(mu, std).log_prob(u)
            na = torch.tanh(u)
            logp = logp - torch.log(1 - torch.tanh(na).pow(2) + 1e-7)
            entropy = -logp.sum(dim=1, keepdim=True)
            q = torch.min(mods[i][1][0](x, na * MAX_DELTA), mods[i][1][1](x, na * MAX_DELTA))
            torch.mean(-twin_leaves[i].exp().detach() * entropy - q).backward(inputs=list(twins[i].parameters()))
            torch.mean((entropy - (-float(aw))).detach() * twin_leaves[i].exp()).backward(inputs=[twin_leaves[i]])
        opt.step()
        opt_alpha.step()
    now = snapshot(sac)
    assert same(now["online"], start["online"]) and not same(now["actor"], start["actor"])
    worst = 0.0
    for i in range(len(agents)):
        views = sac.actors.parameters(i)
        for k, p in mods[i][0].named_parameters():
            assert p.data_ptr() == views[k].data_ptr()                                    # no copy: the module reads the pack
            twin_p = dict(twins[i].named_parameters())[k]
            moved = (twin_p - torch.as_tensor(unpack(sac.actors.offsets, start["actor"])[i][k]).cuda()).abs().max().item()
            err = (p - twin_p).abs().max().item()
            worst = max(worst, err)
            print(f"agent {i} {k}: moved by {moved:.3g}, differs from torch's by {err:.3g}")
            # Adam moves an element by about lr per step against its gradient's sign: a wrong sign or scale is an error of the order of
            # steps * lr.  Where a gradient is all rounding error its sign is, too, and torch's own step is no better defined
            clear = twin_p.grad.abs() > 1e-4 * twin_p.grad.abs().max()
            assert clear.any() and torch.allclose(p[clear], twin_p[clear], rtol=0, atol=0.2 * lr), (i, k, (p - twin_p)[clear].abs().max().item())
        assert leaves[i].data_ptr() == sac.log_alpha[i:i + 1].data_ptr()
        err = abs(leaves[i].item() - twin_leaves[i].item())
        print(f"agent {i} log_alpha: moved by {abs(twin_leaves[i].item() - float(c['log_alpha'][i])):.3g}, differs from torch's by {err:.3g}")
        assert err <= 0.2 * lr
    print(f"largest difference from torch's modules behind {steps} steps: {worst:.3g}")
    # the next act reads the stepped pack
    row = s[:1].contiguous()
    sac.actors.act(row, noise=nz[:1].contiguous())
    for i, (o0, ow, a0, aw) in enumerate(agents):
        mu, _, std = am.forward("sac", unpack(sac.actors.offsets, now["actor"])[i], host(row)[:, :, o0:o0 + ow])
        assert same(host(sac.actors.outputs["mu"])[:, a0:a0 + aw], mu)
        with torch.no_grad():
            assert torch.allclose(mods[i][0](row[:, :, o0:o0 + ow])[0], sac.actors.outputs["mu"][:, a0:a0 + aw], rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------------- with an env
def env_update(torch, how, given, S=5, B=40, iterations=2):
    """An env's store filled by its actors, then the whole update sample -> td_target -> critic_update -> actor_update -> soft_update: one
    warm iteration with the steps switched off (it allocates), then `iterations` recorded ones, eager or as replays of ONE captured graph."""
    from test_gpu_actors import env_actors

    env = nine(8)
    buf = env.replay_store(8, stack_size=S, seed=1)
    actors, _ = env_actors(env, "sac", S)
    sac = env.sac_targets(actors, tau=0.1, seed=5)
    rng = np.random.default_rng(9)
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        for w in ("critic_1", "critic_2", "target_critic_1", "target_critic_2"):
            sac.load_state_dict(aid, w, random_critic(rng, o.stop - o.start, a.stop - a.start, S, scale=1.0))
    env.reset()
    buf.begin()
    for _ in range(7):
        act = actors.act(buf.stacked_obs())
        env.step_device(act, sync=True)
        buf.push(act)
    noise = [torch.as_tensor(rng.standard_normal((B, env.n_actions)).astype(F)).cuda() for _ in range(2)] if given else [None, None]

    def update(step=True):
        s, a, r, ns, d, idx = buf.sample(B)
        td = sac.td_target(r, ns, d, noise=noise[0])
        ca = a.to(torch.float32)
        if step:
            sac.critic_update(s, ca, td, lr=1e-3)
            sac.actor_update(s, noise[1], actor_lr=1e-3, alpha_lr=1e-3)
        else:
            sac.critic_gradients(s, ca, td)
            sac.actor_gradients(s, noise[1])
        sac.soft_update()
        return s

    keep = lambda s: dict(s=host(s).copy(), losses=host(sac.critic_outputs.losses).copy(), critic_adam=host(sac._critic_device()["adam"]).copy(),
                          **outputs(sac), **snapshot(sac))
    log = []
    update(step=False)
    torch.cuda.synchronize()
    draws = sac.actor_draws()
    if how == "graph":
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):                # one stream: the launches in a row
            out = update()
        for _ in range(iterations):
            g.replay()
            torch.cuda.synchronize()
            log.append(keep(out))
    else:
        for _ in range(iterations):
            out = update()
            torch.cuda.synchronize()
            log.append(keep(out))
    assert sac.actor_adam_steps() == iterations and sac.adam_steps() == iterations
    assert sac.actor_draws() == draws + (0 if given else iterations)
    env.close()
    return log


def test_a_captured_whole_update():
    torch = pytest.importorskip("torch")
    eager, graph = env_update(torch, "eager", True), env_update(torch, "graph", True)
    assert len(eager) == len(graph) == 2
    for t, (x, y) in enumerate(zip(eager, graph)):
        assert np.isfinite(x["actor_loss"]).all() and np.isfinite(x["grads"]).all()
        for k in x:
            assert same(x[k], y[k]), (t, k)
    assert not same(eager[0]["actor"], eager[1]["actor"]) and not same(eager[0]["s"], eager[1]["s"])      # every replay samples and steps anew
    assert not same(eager[0]["log_alpha"], eager[1]["log_alpha"])
    # with drawn noise every replay advances the draw counter (asserted in env_update) and draws other numbers
    drawn = env_update(torch, "graph", False)
    assert not same(drawn[0]["eps"], drawn[1]["eps"]) and np.isfinite(drawn[1]["eps"]).all() and np.abs(drawn[1]["eps"]).max() < 7


def test_drawn_noise_is_the_models():
    torch = pytest.importorskip("torch")
    name, S, B = "mixed50", 1, 35
    c = setup(name, S)
    sac = make(name, S, seed=(7 << 32) | 9)
    s = torch.as_tensor(c["ns"][:B]).cuda()
    for d in range(2):
        sac.actor_gradients(s)
        assert sac.actor_draws() == d + 1 and sac.draws() == 0
        want = mm.noise((7 << 32) | 9, np.arange(B)[:, None], np.arange(c["n_actions"])[None, :], d)
        assert same(host(sac.actor_outputs.eps), want), d


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    torch = pytest.importorskip("torch")
    name, S, B = "one", 5, 3
    c = setup(name, S)
    sac = make(name, S, load=False)
    s, nz = (torch.as_tensor(c[k][:B]).cuda() for k in ("ns", "noise"))
    with pytest.raises(ValueError, match="no actor parameters were loaded"):
        sac.actor_update(s, nz)
    sac.actors.load_state_dict(0, c["actors"][0])
    with pytest.raises(ValueError, match="no critics were loaded"):
        sac.actor_update(s, nz)
    sac.load_state_dict(0, "critic_1", c["critics"][0]["critic_1"])
    with pytest.raises(ValueError, match="no critics were loaded.*critic_2"):
        sac.actor_gradients(s, nz)
    sac.load_state_dict(0, "critic_2", c["critics"][0]["critic_2"])
    for bad in (s[:, :2], s.double(), s.transpose(1, 2), s.view(B, -1), s.cpu(), host(s)):
        with pytest.raises(ValueError, match="states must"):
            sac.actor_update(bad, nz)
    for bad in (nz[:2], nz.double(), nz.cpu(), torch.zeros(B, 2, device="cuda"), torch.zeros(B, 2, device="cuda")[:, :1]):
        with pytest.raises(ValueError, match="noise must"):
            sac.actor_update(s, bad)
    with pytest.raises(ValueError, match="lr"):
        sac.actor_update(s, nz, actor_lr=float("nan"))
    with pytest.raises(ValueError, match="lr"):
        sac.actor_update(s, nz, alpha_lr=-1.0)
    with pytest.raises(ValueError, match="betas"):
        sac.actor_update(s, nz, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="target_entropy must be finite"):
        sac.actor_update(s, nz, target_entropy=float("inf"))
    with pytest.raises(ValueError, match="target_entropy must be a number or 1 numbers"):
        sac.actor_update(s, nz, target_entropy=[-1.0, -2.0])
    with pytest.raises(ValueError, match="actor_update\\(\\) has not run"):
        sac.actor_outputs
    assert sac.actor_adam_steps() == 0
    sac.actor_update(s, nz)                                   # the target critics are not needed
    assert sac.actor_adam_steps() == 1 and sac.actor_draws() == 0 and sac.adam_steps() == 0
    exp_avg, exp_avg_sq = sac.actor_adam_state(0)
    assert list(exp_avg) == list(sac.actors.parameters(0)) + ["log_alpha"] and exp_avg["fc.weight"].shape == (64, 64)
    assert exp_avg["fc.weight"].abs().max().item() > 0 and exp_avg_sq["fc.weight"].min().item() >= 0 and exp_avg["log_alpha"].abs().item() > 0
    sac.reset_actor_adam()
    assert sac.actor_adam_steps() == 0 and exp_avg["fc.weight"].abs().max().item() == 0 and exp_avg["log_alpha"].item() == 0
