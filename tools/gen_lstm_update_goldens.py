"""Record what the epochs of the reference's PPOAgent.update() compute with its default, recurrent agents (use_stacked_obs=False;
rl/agents/PPO_org.py:579-629, the KL stop at :752-755), one trajectory per case: tests/golden/lstmup_<case>_*.npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  tools/gen_ppo_update_goldens.py's scheme with tools/gen_lstm_goldens.py's agent: the
reference's own PPOAgent(obs_dim, act_dim, use_delta_actions=True) is constructed at section 17's shapes and fed a trajectory of T = 37
rows through its stateful take_action / store_transition; then update() is CALLED with EPOCHS epochs.  A pre-hook on actor_optimizer.step
(both backward passes and both clip_grad_norm_ calls are behind it, no step yet) records per epoch the parameters and the clipped
gradients of both networks, recomputes the epoch in float32 on copies of the modules (asserting the recorded gradients BIT FOR BIT, which
pins the inputs the tool formed: old_log_probs, the normalised advantage, td_target) and in float64 on copies converted to double; a
post-hook on critic_optimizer.step records the stepped parameters and Adam state of both and steps a float64 Adam, whose state is copied
from the float32 optimiser's, on the recorded float32 gradients.  Only inputs and recorded results are stored, float64 results as
float32(x32 - x64):

    lstmup_<case>_in.npz              obs [T + 1, obs_dim], actions, old_log_probs [T, act_dim], advantage, td_target [T], info_json
    lstmup_<case>_e<k>_<net>_grad.npz   p.<key> (before the step), g.<key> (clipped), dg.<key>, post.<key>, dpost.<key>; the net's forward
                                      (actor: log_probs, mu, std; value: values) and scalars (loss, approx_kl, norm, coef), each x and dx
    lstmup_<case>_e<k>_<net>_adam.npz   m.<key>, dm.<key>, v.<key>, dv.<key> behind the step

The tool, not the test, makes the comparison mean something and asserts: some recorded epoch of every case has elements in each class
(ratio inside the range: a tie; outside with surr1 selected; outside with surr2 selected) and every element falls in the same class in
float32 and float64; advantages of both signs; across the cases clip_grad_norm_ both scales and leaves alone, every norm at least 100
times its float32 error from max_norm; one case stops early and the others run all epochs, every approx_kl at least 100 times its
float32 error from 1.5 kl_tolerance; 0.05 <= std <= 10; epoch 0's ratios are within 1e-5 of 1 (not exactly 1: see record()); some activated gate of every case lies beyond
0.99 or below 0.01.

    python tools/gen_lstm_update_goldens.py
"""
import copy
import json
import os
import sys

os.environ.setdefault("MKL_CBWR", "AVX2,STRICT")       # tools/gen_ppo_eval_goldens.py says why

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_harness as rh  # noqa: E402,F401  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

from gen_actor_goldens import modules  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
T, MAX_DELTA, EPOCHS, MAX_NORM = 37, 2.5, 3, 0.5
CASES = ((4, 1), (20, 4), (56, 8), (6, 2))                     # section 17's shapes: obs_dim, act_dim
# per case: actor_lr (large enough that a step moves ratios out of [0.8, 1.2]), critic_lr, kl_tolerance (the first case's approx_kl behind
# its first step is +0.0096: its tolerance puts the stop behind epoch 1's step), the rewards' scale; SCALES: the
# parameters' scale (the last case's is scaled DOWN so that its gradient norms stay below max_norm and clip_grad_norm_ leaves alone)
HYPER = ((3e-2, 6e-4, 3e-3, 1.0), (1e-2, 6e-4, 10.0, 1.0), (3e-3, 6e-4, 10.0, 1.0), (3e-2, 6e-4, 10.0, 0.02))
SCALES = ((4.0, 1.0), (3.0, 3.0), (3.0, 3.0), (4.0, 0.05))                 # (the lstm.* tensors, the heads)
F = np.float32


def epoch(torch, actor, value, states, actions, old, adv, td, clip_eps):
    """One epoch's forward, losses, backward and clipping on the given modules, lines 583-626; returns the recorded pieces."""
    from torch.distributions import Normal

    mu, std, _ = actor(states.unsqueeze(0))
    mu, std = mu.squeeze(0), std.squeeze(0)
    log_probs = Normal(mu, std).log_prob(actions)
    ratio = torch.exp((log_probs - old).clamp(-20, 20))
    surr1, surr2 = ratio * adv, torch.clamp(ratio, 1 - clip_eps, 1 + clip_eps) * adv
    actor_loss = torch.mean(-torch.min(surr1, surr2))
    values = value.forward_all_steps(states.unsqueeze(0))[0].squeeze(0)
    critic_loss = torch.mean(torch.nn.functional.mse_loss(values, td))
    actor.zero_grad()
    value.zero_grad()
    actor_loss.backward()
    critic_loss.backward()
    na = torch.nn.utils.clip_grad_norm_(actor.parameters(), max_norm=MAX_NORM)
    nv = torch.nn.utils.clip_grad_norm_(value.parameters(), max_norm=MAX_NORM)
    with torch.no_grad():
        lo, hi = 1 - clip_eps, 1 + clip_eps
        inside = (ratio >= lo) & (ratio <= hi)
        cls = torch.where(inside, 0, torch.where(surr1 < surr2, 1, 2))
        out = {"actor": dict(log_probs=log_probs, mu=mu, std=std, loss=actor_loss, approx_kl=(log_probs - old).mean(), norm=na,
                             coef=torch.clamp(MAX_NORM / (na + 1e-6), max=1.0)),
               "value": dict(values=values[:, 0], loss=critic_loss, norm=nv, coef=torch.clamp(MAX_NORM / (nv + 1e-6), max=1.0))}
        grads = {"actor": {k: p.grad.clone() for k, p in actor.named_parameters()}, "value": {k: p.grad.clone() for k, p in value.named_parameters()}}
    return out, grads, cls, ratio.detach()


def gates_range(torch, net, states):
    """(min, max) of the activated i, f, o gates of the net's LSTM over the sequence from a zero state"""
    with torch.no_grad():
        out, _ = net.lstm(states.unsqueeze(0))
        h_prev = torch.cat([torch.zeros(1, out.shape[2], dtype=out.dtype), out[0, :-1]], dim=0)
        pre = states @ net.lstm.weight_ih_l0.T + net.lstm.bias_ih_l0 + h_prev @ net.lstm.weight_hh_l0.T + net.lstm.bias_hh_l0
        s = torch.sigmoid(torch.cat([pre[:, :128], pre[:, 192:]], dim=1))
    return float(s.min()), float(s.max())


def record(obs_dim, act_dim, scale, k, hyper=None, shift=0, save=True):
    import torch
    from torch.distributions import Normal

    _, ppo = modules()
    rl_utils = sys.modules["rl.rl_utils"]
    actor_lr, critic_lr, kl_tol, rscale = hyper or HYPER[k]
    torch.manual_seed(900 + k + 100 * shift)
    rng = np.random.default_rng(13000 + k + 100 * shift)
    low, high = np.zeros(act_dim, dtype=F), np.full(act_dim, 4.0, dtype=F)
    agent = ppo.PPOAgent(obs_dim, act_dim, low, high, actor_lr=actor_lr, critic_lr=critic_lr, epochs=EPOCHS, kl_tolerance=kl_tol,
                         use_delta_actions=True, max_delta=MAX_DELTA)
    assert not agent.use_stacked_obs and type(agent.actor).__name__ == "LSTMPolicyNetwork" and type(agent.value_net).__name__ == "LSTMValueNetwork"
    with torch.no_grad():
        for net in (agent.actor, agent.value_net):
            for name, p in net.named_parameters():
                p.mul_(scale[0] if name.startswith("lstm.") else scale[1])
    obs = (rng.standard_normal((T + 1, obs_dim)) * 3.0).astype(F)
    rewards = (rng.standard_normal(T) * rscale).astype(F)
    dones = np.zeros(T, dtype=F)
    dones[-1] = 1.0
    agent.reset_buffer()
    with torch.no_grad():
        for t in range(T):
            action = agent.take_action(obs[t])
            agent.store_transition(state=obs[t], action=action, next_state=obs[t + 1], reward=rewards[t], done=bool(dones[t]))
    td_ = agent.transition_dict
    states = torch.tensor(np.array(td_["states"]), dtype=torch.float)
    next_states = torch.tensor(np.array(td_["next_states"]), dtype=torch.float)
    acts = torch.tensor(np.array(td_["actions"])).view(-1, act_dim)
    assert acts.dtype == torch.float32
    r = torch.tensor(np.array(td_["rewards"]), dtype=torch.float).view(-1, 1)
    d = torch.tensor(np.array(td_["dones"]), dtype=torch.float).view(-1, 1)
    with torch.no_grad():                                      # lines 543-577
        next_values = agent.value_net.forward_all_steps(next_states.unsqueeze(0))[0].squeeze(0)
        current = agent.value_net.forward_all_steps(states.unsqueeze(0))[0].squeeze(0)
        td_target = r + agent.gamma * next_values * (1 - d)
        advantage = rl_utils.compute_gae(agent.gamma, agent.lmbda, (td_target - current).cpu())
        advantage = (advantage - advantage.mean()) / (advantage.std() + 1e-8)
        mu, std, _ = agent.actor(states.unsqueeze(0))
        mu, std = mu.squeeze(0), std.squeeze(0)
        old = Normal(mu, std).log_prob(acts)
    assert (advantage > 0).any() and (advantage < 0).any()
    dbl = lambda x: x.double()
    epochs, posts = [], []

    def before_actor_step(opt, args, kwargs):
        a32, v32 = copy.deepcopy(agent.actor), copy.deepcopy(agent.value_net)
        o32, g32, c32, ratio32 = epoch(torch, a32, v32, states, acts, old, advantage, td_target, agent.clip_eps)
        for name, net in (("actor", agent.actor), ("value", agent.value_net)):
            for key, p in net.named_parameters():
                assert torch.equal(p.grad, g32[name][key]), ("the tool's epoch is not update()'s", name, key)
        a64, v64 = copy.deepcopy(agent.actor).double(), copy.deepcopy(agent.value_net).double()
        o64, g64, c64, _ = epoch(torch, a64, v64, dbl(states), dbl(acts), dbl(old), dbl(advantage), dbl(td_target), agent.clip_eps)
        assert torch.equal(c32, c64), "an element changes its class between float32 and float64"
        pre = {name: {key: p.detach().clone() for key, p in net.named_parameters()} for name, net in (("actor", agent.actor), ("value", agent.value_net))}
        state = {}
        for name, net, op in (("actor", agent.actor, agent.actor_optimizer), ("value", agent.value_net, agent.critic_optimizer)):
            state[name] = {key: ((op.state[p]["exp_avg"].clone(), op.state[p]["exp_avg_sq"].clone()) if p in op.state and "exp_avg" in op.state[p]
                                 else (torch.zeros_like(p), torch.zeros_like(p))) for key, p in net.named_parameters()}
        epochs.append(dict(o32=o32, o64=o64, g32=g32, g64=g64, cls=c32, ratio=ratio32, pre=pre, state=state))

    def after_critic_step(opt, args, kwargs):
        e, t = epochs[-1], len(epochs)
        post = {}
        for name, net, op, lr in (("actor", agent.actor, agent.actor_optimizer, actor_lr), ("value", agent.value_net, agent.critic_optimizer, critic_lr)):
            post[name] = {}
            for key, p in net.named_parameters():
                st = op.state[p]
                assert int(st["step"]) == t
                g, (m0, v0), p0 = dbl(e["g32"][name][key]), e["state"][name][key], dbl(e["pre"][name][key])
                m64 = 0.9 * dbl(m0) + (1 - 0.9) * g                       # torch.optim.Adam's step in float64 on the float32 gradient and state
                v64 = 0.999 * dbl(v0) + (1 - 0.999) * g * g
                p64 = p0 - (lr / (1 - 0.9 ** t)) * m64 / (v64.sqrt() / (1 - 0.999 ** t) ** 0.5 + 1e-8)
                post[name][key] = dict(p=p.detach().clone(), m=st["exp_avg"].clone(), v=st["exp_avg_sq"].clone(), p64=p64, m64=m64, v64=v64)
        posts.append(post)

    agent.actor_optimizer.register_step_pre_hook(before_actor_step)
    agent.critic_optimizer.register_step_post_hook(after_critic_step)
    agent.update()
    n = len(epochs)
    assert n == len(posts) and 1 <= n <= EPOCHS
    kls = [float(e["o32"]["actor"]["approx_kl"]) for e in epochs]
    if not save:
        return [float(e["o32"][n]["norm"]) for e in epochs for n in ("actor", "value")], [gates_range(torch, agent.actor, states)], kls, [np.bincount(e["cls"].numpy().ravel(), minlength=3).tolist() for e in epochs]
    stopped = n < EPOCHS
    assert all((kl > 1.5 * kl_tol) == (i == n - 1 and stopped) for i, kl in enumerate(kls)), (kls, kl_tol)
    # (a finding: epoch 0's ratios are NOT exactly 1 in the reference -- its nn.LSTM forward under no_grad, which formed old_log_probs, and
    # the one that records a graph differ in the last bits; the distance is recorded)
    ratio0 = float((epochs[0]["ratio"] - 1).abs().max())
    assert ratio0 < 1e-5, ratio0
    counts = [np.bincount(e["cls"].numpy().ravel(), minlength=3).tolist() for e in epochs]
    assert any(min(c) > 0 for c in counts), ("no epoch has all three classes", counts)
    gmin, gmax = zip(*(gates_range(torch, net, states) for e in epochs for net in [agent.actor, agent.value_net]))
    assert min(gmin) < 0.01 or max(gmax) > 0.99, ("no saturated gate", min(gmin), max(gmax))
    info = {"obs_dim": obs_dim, "act_dim": act_dim, "gates": [min(gmin), max(gmax)], "ratio0_minus_1": ratio0, "scale": scale, "T": T, "actor_lr": actor_lr, "critic_lr": critic_lr,
            "kl_tolerance": kl_tol, "clip_eps": agent.clip_eps, "max_grad_norm": MAX_NORM, "epochs": EPOCHS, "epochs_run": n, "stopped": stopped,
            "classes": counts, "approx_kl": kls, "torch": torch.__version__, "MKL_CBWR": os.environ["MKL_CBWR"], "coefs": [], "norms": []}
    case = f"lstmup_o{obs_dim}_a{act_dim}"
    num = lambda x: x.detach().numpy()
    sizes = []
    for i, (e, post) in enumerate(zip(epochs, posts)):
        s32 = num(e["o32"]["actor"]["std"])
        assert 0.05 <= s32.min() and s32.max() <= 10.0 and agent.actor is not None
        assert abs(kls[i] - 1.5 * kl_tol) >= 100 * abs(kls[i] - float(e["o64"]["actor"]["approx_kl"])), ("approx_kl is too close to the stop", i)
        for name in ("actor", "value"):
            o32, o64 = e["o32"][name], e["o64"][name]
            n32, n64 = float(o32["norm"]), float(o64["norm"])
            assert abs(n32 - MAX_NORM) >= 100 * abs(n32 - n64), ("a norm is too close to max_norm", name, i, n32, n64)
            info["coefs"].append(float(o32["coef"]))
            info["norms"].append(n32)
            out = {}
            for key in e["pre"][name]:
                out["p." + key], out["g." + key] = num(e["pre"][name][key]), num(e["g32"][name][key])
                out["dg." + key] = (num(e["g32"][name][key]).astype(np.float64) - num(e["g64"][name][key])).astype(F)
                out["post." + key] = num(post[name][key]["p"])
                out["dpost." + key] = (num(post[name][key]["p"]).astype(np.float64) - num(post[name][key]["p64"])).astype(F)
            for key, x in o32.items():
                out[key] = num(x).astype(F)
                out["d" + key] = (num(x).astype(np.float64) - num(o64[key])).astype(F)
            path = os.path.join(GOLDEN, f"{case}_e{i}_{name}_grad.npz")
            np.savez_compressed(path, **out)
            sizes.append(os.path.getsize(path))
            out = {}
            for key in e["pre"][name]:
                for tag in ("m", "v"):
                    out[f"{tag}.{key}"] = num(post[name][key][tag])
                    out[f"d{tag}.{key}"] = (num(post[name][key][tag]).astype(np.float64) - num(post[name][key][tag + "64"])).astype(F)
            path = os.path.join(GOLDEN, f"{case}_e{i}_{name}_adam.npz")
            np.savez_compressed(path, **out)
            sizes.append(os.path.getsize(path))
    np.savez_compressed(os.path.join(GOLDEN, f"{case}_in.npz"), obs=obs, actions=num(acts), old_log_probs=num(old), advantage=num(advantage)[:, 0],
                        td_target=num(td_target)[:, 0], info_json=np.array(json.dumps(info)))
    assert max(sizes) <= 666561, max(sizes)
    print(f"{case}: {n} epochs{' (stopped early)' if stopped else ''}, classes {counts}, approx_kl {[f'{v:.3g}' for v in kls]}, norms "
          f"{[f'{v:.3g}' for v in info['norms']]}, largest file {max(sizes)} bytes", flush=True)
    return info


if __name__ == "__main__":
    infos = [record(obs_dim, act_dim, SCALES[k], k) for k, (obs_dim, act_dim) in enumerate(CASES)]
    coefs = [c for i in infos for c in i["coefs"]]
    assert any(c < 1 for c in coefs) and any(c == 1 for c in coefs), "clip_grad_norm_ must both scale and leave alone across the cases"
    assert sum(i["stopped"] for i in infos) == 1, "one case stops early and the others run all epochs"
