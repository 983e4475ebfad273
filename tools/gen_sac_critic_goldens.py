"""Record what the critic half of the reference's SACAgent.update computes for a few random minibatches: tests/golden/saccr_<case>.npz and
tests/golden/saccr_<case>_u<k>_c<c>[_g|_adam].npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  rl.agents.SAC is imported under the bare `rl` package of
oracle/ref_harness.load_reference_rl().  The reference's own SACAgent is constructed and its update(transition_dict) is CALLED; only
inputs and recorded results are stored.  calc_target is wrapped so that the td_target it returns is recorded; step pre- and post-hooks on
critic_1_optimizer and critic_2_optimizer snapshot the parameters, the gradients and the Adam state around the step.  Before every update a
float64 twin of both critics is copied from the float32 parameters; behind the update it runs the same forward and backward on the same
inputs and the recorded td_target (float64), so every comparison is one step from the same start.  A second float64 copy with its own
torch.optim.Adam, whose state is copied from the float32 optimiser's, is fed the recorded FLOAT32 gradients and stepped once: that
isolates the optimiser's arithmetic.

    saccr_<case>.npz
      states [U, B, S, obs_dim], actions [U, B, act_dim], td_target [U, B]   float32, of the U consecutive updates
      q32 [U, 2, B], loss32 [U, 2]; q64, loss64   the reference's float32 values and the twin's float64 values (critic 1, critic 2)
      c1.<key>, c2.<key>     the critics' parameters before the first update (the Adam state is empty there: zeros, step 0)
      lr, beta1, beta2, eps, info_json
    saccr_<case>_u<k>_c<c>.npz     update k (from 0), critic c (1, 2); split into ..._g.npz and ..._adam.npz where one file would exceed
                                   the size limit of a golden
      g32.<key>              the float32 gradients the optimiser's step saw
      gerr.<key>             float32(g32 - g64): the float64 twin's gradient is g32 - gerr (kept so, the volume is half that of float64
                             arrays and the reconstruction is exact to 2^-24 of the ERROR)
      p32, m32, v32 .<key>   parameters, exp_avg, exp_avg_sq behind the float32 step; the parameters and the state BEFORE step k > 0 are
                             those behind step k - 1
      perr, merr, verr .<key>  float32(x32 - x64) against the float64 Adam step on the float32 gradients

Cases (obs_dim, act_dim, S): (4, 1, 4), (20, 4, 5), (6, 2, 1) with three consecutive updates of 64 rows, (40, 8, 5) with one.

    python tools/gen_sac_critic_goldens.py
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


def snapshot(opt):
    """(parameters, gradients, exp_avg, exp_avg_sq, step) of an optimiser's only group, as float arrays (an empty state: zeros, 0)."""
    ps = opt.param_groups[0]["params"]
    arr = lambda t: t.detach().numpy().copy()
    st = [opt.state.get(p, {}) for p in ps]
    return ([arr(p) for p in ps], [arr(p.grad) for p in ps], [arr(s["exp_avg"]) if s else np.zeros_like(arr(p)) for s, p in zip(st, ps)],
            [arr(s["exp_avg_sq"]) if s else np.zeros_like(arr(p)) for s, p in zip(st, ps)], [float(s["step"]) if s else 0.0 for s in st])


def record(obs_dim, act_dim, S, updates, k):
    import torch
    import torch.nn.functional as Fn

    rh.load_reference_rl()
    sac = importlib.import_module("rl.agents.SAC")
    torch.manual_seed(700 + k)
    rng = np.random.default_rng(9700 + k)
    low, high = np.zeros(act_dim, dtype=np.float32), np.full(act_dim, 4.0, dtype=np.float32)
    agent = sac.SACAgent(obs_dim, act_dim, low, high, stack_size=S, hidden_size=64, max_delta=MAX_DELTA)
    with torch.no_grad():                                     # the targets lag behind the online critics
        for net in (agent.target_critic_1, agent.target_critic_2):
            for p in net.parameters():
                p.mul_(1 + 0.1 * torch.randn_like(p))
    critics, opts = (agent.critic_1, agent.critic_2), (agent.critic_1_optimizer, agent.critic_2_optimizer)
    keys = [name for name, _ in agent.critic_1.named_parameters()]
    group = opts[0].param_groups[0]
    assert not group.get("amsgrad") and not group.get("weight_decay") and not group.get("maximize")

    seen = {}
    calc_target = agent.calc_target

    def recording_calc_target(*args):
        seen["td"] = calc_target(*args)
        return seen["td"]

    agent.calc_target = recording_calc_target
    for c, opt in enumerate(opts):
        opt.register_step_pre_hook(lambda o, a, kw, c=c: seen.__setitem__(("pre", c), snapshot(o)))
        opt.register_step_post_hook(lambda o, a, kw, c=c: seen.__setitem__(("post", c), snapshot(o)))

    case = f"o{obs_dim}_a{act_dim}_s{S}"
    main = {f"c{c + 1}.{key}": v.detach().numpy().copy() for c, net in enumerate(critics) for key, v in net.state_dict().items()}
    per_update = {name: [] for name in ("states", "actions", "td_target", "q32", "q64", "loss32", "loss64")}
    sizes = []
    for u in range(updates):
        x = (rng.standard_normal((B, S, obs_dim)) * 3.0).astype(np.float32)
        pick = rng.integers(0, 16, size=x.shape)
        x[pick == 0] = 0.0
        x[pick == 1] = -0.0
        nx = (x + rng.standard_normal(x.shape).astype(np.float32)).astype(np.float32)
        actions = rng.uniform(-MAX_DELTA, MAX_DELTA, size=(B, act_dim)).astype(np.float32)
        rewards = rng.standard_normal(B).astype(np.float32)
        dones = (rng.integers(0, 4, size=B) == 0).astype(np.float32)
        twins = [copy.deepcopy(net).double() for net in critics]
        seen.clear()
        agent.update({"states": x, "actions": actions, "rewards": rewards, "next_states": nx, "dones": dones})      # the reference's own call
        td = seen["td"].detach()
        assert td.dtype == torch.float32 and td.shape == (B, 1)
        xs, ac = torch.tensor(x), torch.tensor(actions)
        q32, q64, loss32, loss64 = [], [], [], []
        for c, (twin, opt) in enumerate(zip(twins, opts)):
            p_pre, g32, m_pre, v_pre, t_pre = seen[("pre", c)]
            p32, _, m32, v32, t_post = seen[("post", c)]
            assert all(t == u for t in t_pre) and all(t == u + 1 for t in t_post)
            assert all(np.array_equal(a.astype(np.float64), b.detach().numpy()) for a, b in zip(p_pre, twin.parameters()))
            # the reference's float32 forward from the parameters before the step (a copy: the live module has been stepped)
            with torch.no_grad():
                before = copy.deepcopy(critics[c])
                for p, v in zip(before.parameters(), p_pre):
                    p.copy_(torch.tensor(v))
                q = before(xs, ac)
                q32.append(q[:, 0].numpy().copy())
                loss32.append(torch.mean(Fn.mse_loss(q, td)).item())
            # the float64 twin: the same forward, loss and backward
            qd = twin(xs.double(), ac.double())
            ld = torch.mean(Fn.mse_loss(qd, td.double()))
            ld.backward()
            q64.append(qd.detach()[:, 0].numpy().copy())
            loss64.append(ld.item())
            g64 = [p.grad.numpy().copy() for p in twin.parameters()]
            # the float64 optimiser on the float32 gradients, from the float32 state
            ps = [torch.nn.Parameter(torch.tensor(v, dtype=torch.float64)) for v in p_pre]
            adam = torch.optim.Adam(ps, lr=group["lr"], betas=group["betas"], eps=group["eps"])
            for p, g, m, v in zip(ps, g32, m_pre, v_pre):
                p.grad = torch.tensor(g, dtype=torch.float64)
                if u:
                    adam.state[p] = {"step": torch.tensor(float(u)), "exp_avg": torch.tensor(m, dtype=torch.float64),
                                     "exp_avg_sq": torch.tensor(v, dtype=torch.float64)}
            adam.step()
            p64 = [p.detach().numpy() for p in ps]
            m64, v64 = [adam.state[p]["exp_avg"].numpy() for p in ps], [adam.state[p]["exp_avg_sq"].numpy() for p in ps]
            err = lambda a32, a64: (a32.astype(np.float64) - a64).astype(np.float32)
            grad, step = {}, {}
            for i, key in enumerate(keys):
                assert g32[i].dtype == np.float32 and g64[i].dtype == np.float64 and p64[i].dtype == np.float64
                grad[f"g32.{key}"], grad[f"gerr.{key}"] = g32[i], err(g32[i], g64[i])
                for tag, a32, a64 in (("p", p32, p64), ("m", m32, m64), ("v", v32, v64)):
                    step[f"{tag}32.{key}"], step[f"{tag}err.{key}"] = a32[i], err(a32[i], a64[i])
            path = os.path.join(GOLDEN, f"saccr_{case}_u{u}_c{c + 1}.npz")
            np.savez_compressed(path, **grad, **step)
            written = [path]
            if os.path.getsize(path) > LIMIT:
                os.remove(path)
                written = [path[:-4] + "_g.npz", path[:-4] + "_adam.npz"]
                np.savez_compressed(written[0], **grad)
                np.savez_compressed(written[1], **step)
            for w in written:
                assert os.path.getsize(w) <= LIMIT, (w, os.path.getsize(w))
                sizes.append(os.path.getsize(w))
        for name, v in (("states", x), ("actions", actions), ("td_target", td[:, 0].numpy().copy()), ("q32", np.stack(q32)), ("q64", np.stack(q64)),
                        ("loss32", np.array(loss32, dtype=np.float32)), ("loss64", np.array(loss64, dtype=np.float64))):
            per_update[name].append(v)
    info = {"obs_dim": obs_dim, "act_dim": act_dim, "stack_size": S, "updates": updates, "batch": B, "keys": keys, "numpy": np.__version__,
            "torch": torch.__version__}
    main.update({name: np.stack(v) for name, v in per_update.items()})
    main.update(lr=np.float64(group["lr"]), beta1=np.float64(group["betas"][0]), beta2=np.float64(group["betas"][1]), eps=np.float64(group["eps"]),
                info_json=np.array(json.dumps(info)))
    path = os.path.join(GOLDEN, f"saccr_{case}.npz")
    np.savez_compressed(path, **main)
    assert os.path.getsize(path) <= LIMIT
    print(f"saccr_{case}: {os.path.getsize(path)} bytes and {len(sizes)} step files of at most {max(sizes)} bytes", flush=True)


if __name__ == "__main__":
    for k, (obs_dim, act_dim, S, updates) in enumerate(SHAPES):
        record(obs_dim, act_dim, S, updates, k)
