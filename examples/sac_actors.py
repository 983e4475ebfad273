"""The decision on the device too: the loop of examples/sac_replay.py with the reference-shaped SAC actor of every agent
(rl/agents/SAC.py:72-107: four 64-wide layers on the stack of the last five observations, tanh * max_delta, delta actions on the gate
widths) evaluated for all envs and all agents by ONE launch inside the captured step (``VecPedNetEnv.stacked_actors``).  The actors are
torch modules of this package (``pednstream_amd.policy.make_module``) whose parameters are bound to the pack the kernel reads: the Adam
step below updates what the next captured decision uses, with no copy.  The update itself is a small behaviour-cloning-style stand-in
of this example's own (not the reference's SAC losses, critics, checkpoints or plots).

    python examples/sac_actors.py [dataset] [n_envs] [policy_steps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.policy import make_module  # noqa: E402
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402

STACK, BATCH, SEED = 5, 64, 4


def build(dataset, n_envs):
    np.random.seed(0)                               # (the scenario's demand is drawn from numpy's global stream: the same for both rollouts)
    env = VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3")
    buf = env.replay_store(capacity=64, stack_size=STACK, seed=0)
    actors = env.stacked_actors(kind="sac", stack_size=STACK, delta_actions=True, max_delta=2.5, seed=SEED)
    torch.manual_seed(0)
    mods = {}
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        mods[aid] = actors.bind(aid, make_module("sac", o.stop - o.start, a.stop - a.start, STACK).to("cuda"))
    return env, buf, actors, mods


def rollout(dataset, n_envs, steps, replayed, train=False):
    """``steps`` policy steps; the actions of every step (host copies).  replayed: the captured graph, else the same calls made eagerly."""
    env, buf, actors, mods = build(dataset, n_envs)
    opt = torch.optim.Adam([p for m in mods.values() for p in m.parameters()], lr=1e-4)
    roll = env.capture(lambda obs: actors.act(buf.stacked_obs()), on_step=lambda obs, rew: buf.push(actors.actions))
    env.reset()
    buf.begin()
    log, updates = [], 0
    for t in range(steps):
        if replayed:
            roll.step()
        else:
            a = actors.act(buf.stacked_obs())
            env.step_device(a, sync=True)
            buf.push(a)
        torch.cuda.synchronize()
        log.append(actors.actions.cpu().numpy().copy())
        if train and t >= 8 and t % 4 == 0:
            # minibatches of stacked transitions, per agent; the loss pulls mu towards the deltas that were rewarded above the batch mean
            loss = 0.0
            for i, aid in enumerate(env.possible_agents):
                s, a, r, ns, d, _ = buf.sample(BATCH, agent=aid)
                mu, std = mods[aid](s)
                width = s[:, -1].reshape(BATCH, a.shape[1], -1)[:, :, -1]
                weight = (r - r.mean()).clamp(min=0).unsqueeze(1)
                loss = loss + (weight * (torch.tanh(mu) * 2.5 - (a.float() - width)).square()).mean() + 1e-3 * std.mean()
            opt.zero_grad()
            loss.backward()
            opt.step()                                  # in place, on the pack: the next captured decision reads the new weights
            updates += 1
    info = (f"{roll.replays} replayed, {roll.eager_steps} eager" if replayed else "eager calls") + f", {actors.draws()} draws, {updates} updates"
    buf.close()
    env.close()
    return log, info, len(mods)


def main():
    dataset = sys.argv[1] if len(sys.argv) > 1 else "nine_intersections"
    n_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    for train in (False, True):
        a, info_a, n = rollout(dataset, n_envs, steps, True, train)
        b, info_b, _ = rollout(dataset, n_envs, steps, False, train)
        same = all((x.view("uint64") == y.view("uint64")).all() for x, y in zip(a, b))
        print(f"{dataset} x {n_envs} envs, {n} actors in one launch per step, {steps} policy steps{' with Adam steps on the bound modules' if train else ''}: "
              f"[{info_a}] vs [{info_b}]: the replayed rollout and the eager one gave the same bits: {same}")
        print(f"  last actions of env 0: {a[-1][0][:6]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
