"""The SAC critic step on the device (pednstream_amd/sac.py: critic_update, critic_gradients; pednstream_amd/csrc/pedn_critic.hpp) against
the contract's numpy restatement (tests/sac_critic_model.py): plain tensors, bound torch modules, a captured update and an env's store.  The
checks are staged like test_gpu_actors.check_outputs: what the contract evaluates in float32 is compared bit for bit, what it evaluates in
float64 and rounds once (Adam's two step scalars, which enter the parameters only) within 2 ulps, and every later stage is fed the
kernel's own earlier outputs.  The tables and the minibatches are test_gpu_sac_targets': its next states serve as states, its noise as the
stored actions and its rewards as the TD targets."""
import numpy as np
import pytest

import sac_critic_model as cm
import sac_target_model as sm
from test_gpu_actors import host, nine, same
from test_gpu_sac_targets import N_MAX, TABLES, make, random_critic, setup, within_ulps

pytestmark = pytest.mark.gpu

TILE = 32
BATCHES = (1, 3, TILE + 1, 130)       # one row, less than a tile, a tile and a row, many tiles with a ragged last one
F = np.float32
ONLINE = ("critic_1", "critic_2")


def unpack(sac, flat):
    """[agent][critic] = {key: array} of a host copy of a pack"""
    return [[{k: flat[at:at + int(np.prod(shape))].reshape(shape) for k, (at, shape) in cur.items()} for cur in pair] for pair in sac.offsets]


def padding(sac):
    pad = np.ones(sac.pack_size, dtype=bool)
    for pair in sac.offsets:
        for cur in pair:
            for at, shape in cur.values():
                pad[at:at + int(np.prod(shape))] = False
    return pad


def snapshot(sac):
    d, cd = sac._device(), sac._critic_device()
    return {"online": host(d["online"]).copy(), "target": host(d["target"]).copy(), "exp_avg": host(cd["exp_avg"]).copy(),
            "exp_avg_sq": host(cd["exp_avg_sq"]).copy(), "adam": host(cd["adam"]).copy(), "grads": host(cd["grads"]).copy()}


def check_forward_and_gradients(sac, agents, before, s, a, td, what=""):
    """q1, q2, the losses and the gradient pack of the last launch against the model on the parameters `before` (a host copy of the
    online pack): bit for bit."""
    out = sac.critic_outputs
    q, losses, grads = (host(out.q1), host(out.q2)), host(out.losses), unpack(sac, host(sac._critic_device()["grads"]))
    params = unpack(sac, before)
    B = s.shape[0]
    assert q[0].shape == (B, len(agents)) and losses.shape == (len(agents), 2)
    for i, (o0, ow, a0, aw) in enumerate(agents):
        for c in range(2):
            g, loss, qm = cm.gradients(params[i][c], s[:, :, o0:o0 + ow], a[:, a0:a0 + aw], td[:, i])
            assert same(q[c][:, i], qm), (what, "q", i, c)
            assert same(losses[i, c], loss), (what, "loss", i, c, losses[i, c], loss)
            for k in g:
                assert same(grads[i][c][k], g[k]), (what, "gradient", i, c, k, np.abs(grads[i][c][k] - g[k]).max())
            views = out.grads(sac.agent_ids[i], ONLINE[c])
            assert list(views) == list(params[i][c]) and set(views) == set(g) and all(same(host(views[k]), grads[i][c][k]) for k in g)


def check_adam(sac, before, t, hyper, what=""):
    """exp_avg, exp_avg_sq (bit for bit) and the online pack (2 ulps: the step scalars) behind step t against the model on the state
    `before` and the launch's own gradient pack; the padding stays +0.0."""
    now = snapshot(sac)
    p, m, v = cm.adam(before["online"], now["grads"], before["exp_avg"], before["exp_avg_sq"], t, **hyper)
    assert same(now["exp_avg"], m), (what, "exp_avg", t)
    assert same(now["exp_avg_sq"], v), (what, "exp_avg_sq", t)
    assert within_ulps(now["online"], p, 2), (what, "parameters", t, np.abs(now["online"] - p).max())
    assert same(now["target"], before["target"]), (what, "the target pack was touched")
    assert now["adam"][0] == t and now["adam"][1] == 0
    want = [1.0, 1.0]
    for _ in range(t):
        want = [want[0] * hyper["betas"][0], want[1] * hyper["betas"][1]]
    assert now["adam"][2:].view(np.float64).tolist() == want      # the running products, in double
    pad = padding(sac)
    for k in ("online", "grads", "exp_avg", "exp_avg_sq"):
        assert pad.any() and not now[k][pad].view(np.uint32).any(), (what, "padding", k)
    return now


# ---------------------------------------------------------------------------------------------------- plain tensors
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("name", list(TABLES))
def test_kernel_equals_the_model(name, S):
    torch = pytest.importorskip("torch")
    c = setup(name, S)
    agents = c["agents"]
    sac = make(name, S)
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)      # (a step large enough to move every parameter by many ulps)
    start = snapshot(sac)
    whole_q = None
    for B in reversed(BATCHES):
        s, a, td = c["ns"][:B], c["noise"][:B], c["rewards"][:B]
        ds, da, dtd = dev(s), dev(a), dev(td)
        # the launches with the Adam step switched off write nothing but their outputs
        sac.critic_gradients(ds, da, dtd)
        after = snapshot(sac)
        for k in ("online", "target", "exp_avg", "exp_avg_sq", "adam"):
            assert same(after[k], start[k]), (B, k)
        check_forward_and_gradients(sac, agents, start["online"], s, a, td, what=("gradients", B))
        q = (host(sac.critic_outputs.q1).copy(), host(sac.critic_outputs.q2).copy())
        if B == N_MAX:
            whole_q = q
        else:                                                 # q of a row does not depend on the batch
            assert same(q[0], whole_q[0][:B]) and same(q[1], whole_q[1][:B]), B
        # three updates, each checked from the state the launch found
        before = after
        for t in (1, 2, 3):
            sac.critic_update(ds, da, dtd, **hyper)
            if t == 1:
                assert same(host(sac._critic_device()["grads"]), after["grads"]), B      # the same gradients with the step switched on
            else:
                check_forward_and_gradients(sac, agents, before["online"], s, a, td, what=("update", B, t))
            before = check_adam(sac, before, t, hyper, what=B)
        assert sac.adam_steps() == 3 and not same(before["online"], start["online"])
        again = sac.critic_outputs
        sac.critic_gradients(ds, da, dtd)
        assert again.q1.data_ptr() == sac.critic_outputs.q1.data_ptr()      # allocated once per batch size
        # back to the start for the next batch size
        sac._device()["online"].copy_(torch.as_tensor(start["online"]))
        sac.reset_adam()
        assert sac.adam_steps() == 0
        for k, v in snapshot(sac).items():
            if k != "grads":
                assert same(v, start[k]), k
    # row position: row 77 of the 130-row launch alone, as row 0 of a launch of one
    sac.critic_gradients(dev(c["ns"][77:78]), dev(c["noise"][77:78]), dev(c["rewards"][77:78]))
    assert same(host(sac.critic_outputs.q1), whole_q[0][77:78]) and same(host(sac.critic_outputs.q2), whole_q[1][77:78])


def test_rows_behind_the_batch_and_awkward_values():
    """A ragged last tile reads nothing behind the batch: the tensors of a 33-row launch are views of larger ones whose later rows are
    NaN.  A NaN inside the batch reaches the sums of its agent and of no other."""
    torch = pytest.importorskip("torch")
    name, S, B = "mixed", 5, TILE + 1
    c = setup(name, S)
    sac = make(name, S)
    start = snapshot(sac)
    s, a, td = (torch.as_tensor(c[k][:B + 40].copy()).cuda() for k in ("ns", "noise", "rewards"))
    s[B:], a[B:], td[B:] = float("nan"), float("inf"), float("nan")
    sac.critic_gradients(s[:B], a[:B], td[:B])
    check_forward_and_gradients(sac, c["agents"], start["online"], c["ns"][:B], c["noise"][:B], c["rewards"][:B])
    assert np.isfinite(host(sac._critic_device()["grads"])).all()
    clean = host(sac._critic_device()["grads"]).copy()
    o0 = c["agents"][1][0]
    s[B - 1, 2, o0 + 3] = float("nan")                        # one column of agent 1, in the last row
    sac.critic_gradients(s[:B], a[:B], td[:B])
    got, was = unpack(sac, host(sac._critic_device()["grads"])), unpack(sac, clean)
    losses = host(sac.critic_outputs.losses)
    assert np.isnan(losses[1]).all() and np.isfinite(losses[[0, 2]]).all()
    for i in (0, 2):
        for cr in range(2):
            assert all(same(got[i][cr][k], was[i][cr][k]) for k in got[i][cr])
    assert all(np.isnan(got[1][cr]["fc_out.bias"]).all() for cr in range(2))
    check_forward_and_gradients(sac, c["agents"], start["online"], host(s[:B]), c["noise"][:B], c["rewards"][:B])


# ---------------------------------------------------------------------------------------------------- bound modules
def test_bound_modules_see_the_step_and_soft_update_reads_it():
    torch = pytest.importorskip("torch")
    from pednstream_amd.sac import WHICH, make_critic_module

    name, S, B = "mixed50", 5, 40
    c = setup(name, S)
    agents = c["agents"]
    sac = make(name, S, tau=0.25)
    torch.manual_seed(2)
    s, a, td = (torch.as_tensor(c[k][:B]).cuda() for k in ("ns", "noise", "rewards"))
    mods, twins = [], []
    for i, (o0, ow, a0, aw) in enumerate(agents):
        four = [make_critic_module(ow, aw, S).cuda() for _ in WHICH]
        sac.bind(i, *four)
        mods.append(four)
        twins.append([make_critic_module(ow, aw, S).cuda() for _ in range(2)])
        for twin, m in zip(twins[-1], four[:2]):
            twin.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    # torch's own backward and Adam on copies of the modules: the same step up to the order of the sums
    opt = torch.optim.Adam([p for pair in twins for m in pair for p in m.parameters()], lr=1e-2)
    for i, (o0, ow, a0, aw) in enumerate(agents):
        for m in twins[i]:
            torch.nn.functional.mse_loss(m(s[:, :, o0:o0 + ow], a[:, a0:a0 + aw]), td[:, i:i + 1]).backward()
    before = snapshot(sac)
    sac.critic_update(s, a, td, lr=1e-2)
    for i in range(len(agents)):
        for cr, (which, m) in enumerate(zip(WHICH[:2], mods[i][:2])):
            views, grads = sac.parameters(i, which), sac.critic_outputs.grads(i, which)
            for k, p in m.named_parameters():
                assert p.data_ptr() == views[k].data_ptr()                                # no copy: the module reads the pack
                twin_p = dict(twins[i][cr].named_parameters())[k]
                assert torch.allclose(grads[k], twin_p.grad, rtol=1e-3, atol=1e-5 * twin_p.grad.abs().max().item()), (i, which, k)
    opt.step()
    after = snapshot(sac)
    assert not same(after["online"], before["online"]) and same(after["target"], before["target"])
    for i in range(len(agents)):
        for cr, m in enumerate(mods[i][:2]):
            for k, p in m.named_parameters():
                twin_p = dict(twins[i][cr].named_parameters())[k]
                # Adam's first step moves an element by lr against its gradient's sign: a wrong sign or scale is an error of 1e-2.  Where
                # the gradient is all rounding error its sign is, too: those elements are left out
                clear = twin_p.grad.abs() > 1e-4 * twin_p.grad.abs().max()
                assert clear.any() and torch.allclose(p[clear], twin_p[clear], rtol=0, atol=2e-3), (i, cr, k, (p - twin_p)[clear].abs().max().item())
    check_forward_and_gradients(sac, agents, before["online"], c["ns"][:B], c["noise"][:B], c["rewards"][:B])
    sac.soft_update()                                         # reads the stepped online critics
    assert same(host(sac._device()["target"]), sm.polyak(before["target"], after["online"], 0.25))
    assert same(host(mods[0][2].fc.weight), host(sac.parameters(0, "target_critic_1")["fc.weight"]))


# ---------------------------------------------------------------------------------------------------- with an env
def env_update(torch, how, S=5, B=40, iterations=3):
    """An env's store filled by its actors, then sample -> td_target -> critic_update -> soft_update: one warm iteration with the Adam
    step switched off (it allocates), then `iterations` recorded ones, eager or as replays of ONE captured graph."""
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
    start = snapshot(sac)
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)

    def update(step=True):
        s, a, r, ns, d, idx = buf.sample(B)
        td = sac.td_target(r, ns, d)
        ca = a.to(torch.float32)                              # (the whole-row stored actions as the critics' inputs)
        (sac.critic_update if step else sac.critic_gradients)(s, ca, td, **(hyper if step else {}))
        sac.soft_update()
        return s, ca, td

    keep = lambda s, ca, td: dict(s=host(s).copy(), a=host(ca).copy(), td=host(td).copy(), q1=host(sac.critic_outputs.q1).copy(),
                                  losses=host(sac.critic_outputs.losses).copy(), **snapshot(sac))
    log = []
    update(step=False)
    torch.cuda.synchronize()
    if how == "graph":
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):                # one stream: the launches in a row
            out = update()
        for _ in range(iterations):
            g.replay()
            torch.cuda.synchronize()
            log.append(keep(*out))
    else:
        for _ in range(iterations):
            out = update()
            torch.cuda.synchronize()
            log.append(keep(*out))
    assert sac.adam_steps() == iterations
    info = dict(agents=sac.agents, start=start, hyper=hyper, sac=sac, pad=padding(sac))
    env.close()
    return log, info


def test_an_envs_minibatch_and_a_captured_update():
    torch = pytest.importorskip("torch")
    eager, info = env_update(torch, "eager")
    first = eager[0]
    assert first["s"].shape[0] == 40 and np.isfinite(first["td"]).all() and np.isfinite(first["losses"]).all() and first["losses"].min() > 0
    # the env's own table: the first update against the model, from the loaded parameters
    sac = info["sac"]
    params, grads = unpack(sac, info["start"]["online"]), unpack(sac, first["grads"])
    for i, (o0, ow, a0, aw) in enumerate(info["agents"]):
        for c in range(2):
            g, loss, q = cm.gradients(params[i][c], first["s"][:, :, o0:o0 + ow], first["a"][:, a0:a0 + aw], first["td"][:, i])
            assert same(first["losses"][i, c], loss) and (c or same(first["q1"][:, i], q)), (i, c)
            assert all(same(grads[i][c][k], g[k]) for k in g), (i, c)
    p, m, v = cm.adam(info["start"]["online"], first["grads"], info["start"]["exp_avg"], info["start"]["exp_avg_sq"], 1, **info["hyper"])
    assert same(first["exp_avg"], m) and same(first["exp_avg_sq"], v) and within_ulps(first["online"], p, 2)
    assert not first["online"][info["pad"]].view(np.uint32).any()
    graph, _ = env_update(torch, "graph")
    assert len(eager) == len(graph) == 3
    for t, (x, y) in enumerate(zip(eager, graph)):
        for k in x:
            assert same(x[k], y[k]), (t, k)
    assert not same(eager[0]["online"], eager[2]["online"]) and not same(eager[0]["s"], eager[1]["s"])      # every replay samples and steps anew


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    torch = pytest.importorskip("torch")
    name, S, B = "one", 5, 3
    c = setup(name, S)
    sac = make(name, S, load=False)
    s, a, td = (torch.as_tensor(c[k][:B]).cuda() for k in ("ns", "noise", "rewards"))
    with pytest.raises(ValueError, match="no critics were loaded"):
        sac.critic_update(s, a, td)
    for which in ("target_critic_1", "target_critic_2", "critic_1"):
        sac.load_state_dict(0, which, c["critics"][0][which])
    with pytest.raises(ValueError, match="no critics were loaded.*critic_2"):
        sac.critic_gradients(s, a, td)
    sac.load_state_dict(0, "critic_2", c["critics"][0]["critic_2"])
    for bad in (s[:2], s.double(), s.transpose(1, 2), s.view(B, -1), s.cpu(), host(s)):
        with pytest.raises(ValueError, match="states must"):
            sac.critic_update(bad, a, td)
    for bad in (a[:2], a.double(), a.cpu(), torch.zeros(B, 2, device="cuda"), torch.zeros(B, 2, device="cuda")[:, :1]):
        with pytest.raises(ValueError, match="actions must"):
            sac.critic_update(s, bad, td)
    for bad in (td.double(), td.cpu(), td.view(-1), torch.zeros(B, 2, device="cuda")[:, :1], torch.zeros(B, 2, device="cuda")):
        with pytest.raises(ValueError, match="td_target must"):
            sac.critic_update(s, a, bad)
    with pytest.raises(ValueError, match="lr"):
        sac.critic_update(s, a, td, lr=float("nan"))
    with pytest.raises(ValueError, match="betas"):
        sac.critic_update(s, a, td, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="critic_update\\(\\) has not run"):
        sac.critic_outputs
    with pytest.raises(ValueError, match="only the online critics"):
        sac.critic_gradients(s, a, td) or sac.critic_outputs.grads(0, "target_critic_1")
    assert sac.adam_steps() == 0
    sac.critic_update(s, a, td)                               # the actors' parameters are not needed
    assert sac.adam_steps() == 1 and sac.draws() == 0
    exp_avg, exp_avg_sq = sac.adam_state(0, "critic_2")
    assert list(exp_avg) == list(sac.parameters(0, "critic_2")) and exp_avg["fc.weight"].shape == (64, 66)
    assert exp_avg["fc.weight"].abs().max().item() > 0 and exp_avg_sq["fc.weight"].min().item() >= 0
    sac.reset_adam()
    assert sac.adam_steps() == 0 and exp_avg["fc.weight"].abs().max().item() == 0
