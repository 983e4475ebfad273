"""Record what the actor half of the reference's SACAgent.update computes for a few random minibatches: tests/golden/sacac_<case>.npz and
tests/golden/sacac_<case>_u<k>[_in|_g|_adam].npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  rl.agents.SAC is imported under the bare `rl` package of
oracle/ref_harness.load_reference_rl().  The reference's own SACAgent is constructed with target_entropy = -act_dim (what its trainer
passes) and its update(transition_dict) is CALLED; only inputs and recorded results are stored.  Step pre- and post-hooks on actor_optimizer
and log_alpha_optimizer snapshot the parameters, the gradients and the Adam state around the step; a post-hook on critic_2_optimizer
snapshots the stepped critics (which the actor loss reads) and torch's RNG state, from which the actor's eps is drawn again behind the
update (the call Normal.rsample makes).  The tool asserts that a float32 torch recomputation of SAC.py:347-370 with that eps, on the actor
before the step and the stepped critics, reproduces the recorded float32 actor gradients and the log_alpha gradient bit for bit.  A float64
twin of the actor and the critics runs the same forward and backward with the same eps, and a float64 torch.optim.Adam whose state is copied
from the float32 optimiser's is fed the recorded FLOAT32 gradients and stepped once: that isolates the optimiser's arithmetic.

The tool also asserts what makes the comparison mean something: every row selects the same critic in float32 and in float64 (the smallest
|q1 - q2| of a case is recorded; critic 2 is perturbed so that it is far above q's float32 error), both critics are selected in every
update, and 0.05 <= std <= 20 (section 15's guard).

    sacac_<case>.npz
      states [U, B, S, obs_dim], eps [U, B, act_dim], log_alpha [U] (before update u), target_entropy   float32
      <name>32, <name>err = float32(x32 - x64) for mu, std, logp [U, B, act_dim], entropy, q1, q2 [U, B], actor_loss, alpha_loss, alpha_grad [U]
      actor.<key>            the actor's parameters before the first update (the Adam state is empty there: zeros, step 0)
      lr, alpha_lr, beta1, beta2, eps_adam, max_delta, info_json
    sacac_<case>_u<k>.npz     update k (from 0); split into ..._in.npz, ..._g.npz and ..._adam.npz where one file would exceed the size limit
      c1.<key>, c2.<key>     the stepped critics the actor loss of update k reads
      g32.<key>, gerr.<key>  the float32 actor gradients the optimiser's step saw, and float32(g32 - g64) against the float64 twin's
      p32, m32, v32 .<key>   parameters, exp_avg, exp_avg_sq behind the float32 step, with perr, merr, verr = float32(x32 - x64) against the
                             float64 Adam step on the float32 gradients; key "log_alpha" holds the temperature's (its errors in float64)

Cases (obs_dim, act_dim, S): (4, 1, 4), (20, 4, 5), (6, 2, 1) with three consecutive updates of 64 rows, (40, 8, 5) with one.

    python tools/gen_sac_actor_goldens.py
"""
import copy
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = ((4, 1, 4, 3), (20, 4, 5, 3), (6, 2, 1, 3), (40, 8, 5, 1))       # obs_dim, act_dim, S, updates
B, MAX_DELTA, LIMIT = 64, 2.5, 666561
FORWARD = ("mu", "std", "logp", "entropy", "q1", "q2", "actor_loss", "alpha_loss", "alpha_grad")


def snapshot(opt):
    """(parameters, gradients, exp_avg, exp_avg_sq, step) of an optimiser's only group, as float arrays (an empty state: zeros, 0)."""
    ps = opt.param_groups[0]["params"]
    arr = lambda t: t.detach().numpy().copy()
    st = [opt.state.get(p, {}) for p in ps]
    return ([arr(p) for p in ps], [arr(p.grad) for p in ps], [arr(s["exp_avg"]) if s else np.zeros_like(arr(p)) for s, p in zip(st, ps)],
            [arr(s["exp_avg_sq"]) if s else np.zeros_like(arr(p)) for s, p in zip(st, ps)], [float(s["step"]) if s else 0.0 for s in st])


def actor_half(torch, actor, c1, c2, log_alpha, target_entropy, bound, states, eps):
    """SAC.py:347-370 line by line with the drawn numbers handed in (Normal.rsample is loc + eps * scale); both backward passes."""
    from torch.distributions import Normal

    mu, std = actor(states)
    dist = Normal(mu, std)
    normal_sample = mu + eps * std
    log_probs = dist.log_prob(normal_sample)
    new_actions = torch.tanh(normal_sample)
    log_probs = log_probs - torch.log(1 - torch.tanh(new_actions).pow(2) + 1e-7)
    new_actions = new_actions * bound
    entropy = -log_probs.sum(dim=1, keepdim=True)
    q1, q2 = c1(states, new_actions), c2(states, new_actions)
    actor_loss = torch.mean(-log_alpha.exp() * entropy - torch.min(q1, q2))
    for p in actor.parameters():
        p.grad = None
    actor_loss.backward(inputs=list(actor.parameters()))
    alpha_loss = torch.mean((entropy - target_entropy).detach() * log_alpha.exp())
    log_alpha.grad = None
    alpha_loss.backward(inputs=[log_alpha])
    out = dict(mu=mu, std=std, logp=log_probs, entropy=entropy[:, 0], q1=q1[:, 0], q2=q2[:, 0], actor_loss=actor_loss, alpha_loss=alpha_loss,
               alpha_grad=log_alpha.grad)
    return {k: v.detach().numpy().copy() for k, v in out.items()}, [p.grad.numpy().copy() for p in actor.parameters()]


def adam64(torch, group, p_pre, g32, m_pre, v_pre, u):
    """One float64 torch.optim.Adam step on the float32 gradients from the float32 state: (p, exp_avg, exp_avg_sq) lists."""
    ps = [torch.nn.Parameter(torch.tensor(v, dtype=torch.float64)) for v in p_pre]
    adam = torch.optim.Adam(ps, lr=group["lr"], betas=group["betas"], eps=group["eps"])
    for p, g, m, v in zip(ps, g32, m_pre, v_pre):
        p.grad = torch.tensor(g, dtype=torch.float64)
        if u:
            adam.state[p] = {"step": torch.tensor(float(u)), "exp_avg": torch.tensor(m, dtype=torch.float64), "exp_avg_sq": torch.tensor(v, dtype=torch.float64)}
    adam.step()
    return [p.detach().numpy() for p in ps], [adam.state[p]["exp_avg"].numpy() for p in ps], [adam.state[p]["exp_avg_sq"].numpy() for p in ps]


def record(obs_dim, act_dim, S, updates, k):
    import torch
    from torch.distributions.utils import _standard_normal

    rh.load_reference_rl()
    sac = importlib.import_module("rl.agents.SAC")
    torch.manual_seed(800 + k)
    rng = np.random.default_rng(9800 + k)
    low, high = np.zeros(act_dim, dtype=np.float32), np.full(act_dim, 4.0, dtype=np.float32)
    target_entropy = -float(act_dim)
    agent = sac.SACAgent(obs_dim, act_dim, low, high, stack_size=S, hidden_size=64, max_delta=MAX_DELTA, target_entropy=target_entropy)
    with torch.no_grad():
        for net in (agent.target_critic_1, agent.target_critic_2):      # the targets lag behind the online critics
            for p in net.parameters():
                p.mul_(1 + 0.1 * torch.randn_like(p))
        for net in (agent.critic_1, agent.critic_2):                    # q's spread over the rows, then critic 2 away from critic 1
            for p in net.parameters():
                p.mul_(2.0)
        for p in agent.critic_2.parameters():
            p.mul_(1 + 0.3 * torch.randn_like(p))
    keys = [name for name, _ in agent.actor.named_parameters()]
    group, alpha_group = agent.actor_optimizer.param_groups[0], agent.log_alpha_optimizer.param_groups[0]
    for g in (group, alpha_group):
        assert not g.get("amsgrad") and not g.get("weight_decay") and not g.get("maximize")
    assert group["betas"] == alpha_group["betas"] and group["eps"] == alpha_group["eps"]

    seen = {}
    for tag, opt in (("actor", agent.actor_optimizer), ("alpha", agent.log_alpha_optimizer)):
        opt.register_step_pre_hook(lambda o, a, kw, tag=tag: seen.__setitem__(("pre", tag), snapshot(o)))
        opt.register_step_post_hook(lambda o, a, kw, tag=tag: seen.__setitem__(("post", tag), snapshot(o)))
    agent.critic_2_optimizer.register_step_post_hook(lambda o, a, kw: seen.update(
        rng=torch.get_rng_state(), c1=copy.deepcopy(agent.critic_1), c2=copy.deepcopy(agent.critic_2)))

    case = f"o{obs_dim}_a{act_dim}_s{S}"
    main = {f"actor.{key}": v.detach().numpy().copy() for key, v in agent.actor.state_dict().items()}
    per_update = {name: [] for name in ("states", "eps", "log_alpha") + tuple(n + t for n in FORWARD for t in ("32", "err"))}
    sizes, margin, lower_rows, std_range = [], np.inf, [], [np.inf, 0.0]
    err = lambda a32, a64: (np.asarray(a32, dtype=np.float64) - np.asarray(a64, dtype=np.float64)).astype(np.float32)
    for u in range(updates):
        x = (rng.standard_normal((B, S, obs_dim)) * 3.0).astype(np.float32)
        pick = rng.integers(0, 16, size=x.shape)
        x[pick == 0] = 0.0
        x[pick == 1] = -0.0
        nx = (x + rng.standard_normal(x.shape).astype(np.float32)).astype(np.float32)
        actions = rng.uniform(-MAX_DELTA, MAX_DELTA, size=(B, act_dim)).astype(np.float32)
        rewards = rng.standard_normal(B).astype(np.float32)
        dones = (rng.integers(0, 4, size=B) == 0).astype(np.float32)
        seen.clear()
        agent.update({"states": x, "actions": actions, "rewards": rewards, "next_states": nx, "dones": dones})      # the reference's own call
        p_pre, g32, m_pre, v_pre, t_pre = seen[("pre", "actor")]
        p32, _, m32, v32, t_post = seen[("post", "actor")]
        (la_pre,), (ga32,), (lam_pre,), (lav_pre,), _ = seen[("pre", "alpha")]
        (la32,), _, (lam32,), (lav32,), _ = seen[("post", "alpha")]
        assert all(t == u for t in t_pre) and all(t == u + 1 for t in t_post)
        # the actor's eps again, from the RNG state in front of its rsample
        after = torch.get_rng_state()
        torch.set_rng_state(seen["rng"])
        eps = _standard_normal((B, act_dim), dtype=torch.float32, device=torch.device("cpu"))       # the call Normal.rsample makes
        torch.set_rng_state(after)
        xs = torch.tensor(x)
        # the reference's float32 arithmetic from the actor before the step and the stepped critics
        before = copy.deepcopy(agent.actor)
        with torch.no_grad():
            for p, v in zip(before.parameters(), p_pre):
                p.copy_(torch.tensor(v))
        la = torch.tensor(la_pre, requires_grad=True)
        out32, again = actor_half(torch, before, seen["c1"], seen["c2"], la, target_entropy, agent.action_bound, xs, eps)
        assert all(a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again, g32)), "not update()'s gradients"
        assert np.array_equal(out32["alpha_grad"].view(np.uint32), ga32.view(np.uint32)), "not update()'s log_alpha gradient"
        # the float64 twin: the same forward and backward with the same eps
        la64 = torch.tensor(la_pre, dtype=torch.float64, requires_grad=True)
        out64, g64 = actor_half(torch, copy.deepcopy(before).double(), copy.deepcopy(seen["c1"]).double(), copy.deepcopy(seen["c2"]).double(), la64,
                                target_entropy, agent.action_bound, xs.double(), eps.double())
        lower32, lower64 = out32["q2"] < out32["q1"], out64["q2"] < out64["q1"]
        assert np.array_equal(lower32, lower64), "a row selects another critic in float64"
        assert lower32.any() and not lower32.all(), "the minimum does not switch between the critics"
        assert 0.05 <= out32["std"].min() and out32["std"].max() <= 20.0, (out32["std"].min(), out32["std"].max())
        q_error = max(np.abs(out32[n] - out64[n]).max() for n in ("q1", "q2"))
        margin = min(margin, float(np.abs(out64["q1"] - out64["q2"]).min()))
        assert margin > 100 * q_error, (margin, q_error)
        lower_rows.append(int(lower32.sum()))
        std_range = [min(std_range[0], float(out32["std"].min())), max(std_range[1], float(out32["std"].max()))]
        # the float64 optimisers on the float32 gradients, from the float32 state
        p64, m64, v64 = adam64(torch, group, p_pre, g32, m_pre, v_pre, u)
        (la64s,), (lam64,), (lav64,) = adam64(torch, alpha_group, [la_pre], [ga32], [lam_pre], [lav_pre], u)
        inputs = {f"c{c}.{key}": v.detach().numpy().copy() for c, net in ((1, seen["c1"]), (2, seen["c2"])) for key, v in net.state_dict().items()}
        grad, step = {}, {}
        for i, key in enumerate(keys):
            assert g32[i].dtype == np.float32 and g64[i].dtype == np.float64 and p64[i].dtype == np.float64
            grad[f"g32.{key}"], grad[f"gerr.{key}"] = g32[i], err(g32[i], g64[i])
            for tag, a32, a64 in (("p", p32, p64), ("m", m32, m64), ("v", v32, v64)):
                step[f"{tag}32.{key}"], step[f"{tag}err.{key}"] = a32[i], err(a32[i], a64[i])
        for tag, a32, a64 in (("p", la32, la64s), ("m", lam32, lam64), ("v", lav32, lav64)):
            step[f"{tag}32.log_alpha"], step[f"{tag}err.log_alpha"] = np.float32(a32), np.float64(a32) - np.float64(a64)
        path = os.path.join(GOLDEN, f"sacac_{case}_u{u}.npz")
        np.savez_compressed(path, **inputs, **grad, **step)
        written = [path]
        if os.path.getsize(path) > LIMIT:
            os.remove(path)
            written = [path[:-4] + "_in.npz", path[:-4] + "_g.npz", path[:-4] + "_adam.npz"]
            for w, part in zip(written, (inputs, grad, step)):
                np.savez_compressed(w, **part)
        for w in written:
            assert os.path.getsize(w) <= LIMIT, (w, os.path.getsize(w))
            sizes.append(os.path.getsize(w))
        per_update["states"].append(x)
        per_update["eps"].append(eps.numpy().copy())
        per_update["log_alpha"].append(np.float32(la_pre))
        for n in FORWARD:
            assert out32[n].dtype == np.float32 and out64[n].dtype == np.float64, n
            per_update[n + "32"].append(out32[n])
            per_update[n + "err"].append(err(out32[n], out64[n]) if out32[n].ndim else np.float64(out32[n]) - out64[n])
    info = {"obs_dim": obs_dim, "act_dim": act_dim, "stack_size": S, "updates": updates, "batch": B, "keys": keys, "smallest_q_margin": margin,
            "q2_lower_rows": lower_rows, "std_min": std_range[0], "std_max": std_range[1], "numpy": np.__version__, "torch": torch.__version__}
    main.update({name: np.stack(v) for name, v in per_update.items()})
    main.update(target_entropy=np.float32(target_entropy), lr=np.float64(group["lr"]), alpha_lr=np.float64(alpha_group["lr"]),
                beta1=np.float64(group["betas"][0]), beta2=np.float64(group["betas"][1]), eps_adam=np.float64(group["eps"]),
                max_delta=np.float64(MAX_DELTA), info_json=np.array(json.dumps(info)))
    path = os.path.join(GOLDEN, f"sacac_{case}.npz")
    np.savez_compressed(path, **main)
    assert os.path.getsize(path) <= LIMIT
    print(f"sacac_{case}: {os.path.getsize(path)} bytes and {len(sizes)} step files of at most {max(sizes)} bytes; smallest |q1 - q2| {margin:.3g}, "
          f"q2 lower in {lower_rows} rows, std in [{std_range[0]:.3g}, {std_range[1]:.3g}]", flush=True)


if __name__ == "__main__":
    for k, (obs_dim, act_dim, S, updates) in enumerate(SHAPES):
        record(obs_dim, act_dim, S, updates, k)
