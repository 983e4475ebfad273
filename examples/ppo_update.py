"""The reference's PPO update (rl/agents/PPO_org.py:518-629) with its gradient-free half on the device: a captured rollout of the stacked
PPO actors fills a rollout store (the replay store only hands the acting stacks out); behind the rows ONE launch evaluates the value
critic of every agent on every state and the old log-probabilities of the stored delta actions (``VecPedNetEnv.ppo_targets``), the store
turns the values into TD targets, GAE and normalised advantages, and a couple of epochs of the reference's clipped loss run in torch on
modules whose parameters are bound to the packs the kernels read.

    python examples/ppo_update.py [dataset] [n_envs] [policy_steps] [epochs]
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Normal

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.policy import make_module  # noqa: E402
from pednstream_amd.ppo import make_value_module  # noqa: E402
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402

STACK, MAX_DELTA, GAMMA, LMBDA, CLIP_EPS = 5, 2.5, 0.99, 0.95, 0.2


def main():
    dataset = sys.argv[1] if len(sys.argv) > 1 else "nine_intersections"
    n_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    epochs = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    np.random.seed(0)
    torch.manual_seed(0)
    env = VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3")
    buf = env.replay_store(capacity=steps + 2, stack_size=STACK, seed=0)        # the acting stacks
    actors = env.stacked_actors(kind="ppo", stack_size=STACK, delta_actions=True, max_delta=MAX_DELTA, seed=4)
    store = env.rollout_store(capacity=steps)
    ppo = env.ppo_targets(actors)
    agents = {}
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        ow, aw = o.stop - o.start, a.stop - a.start
        actor = actors.bind(aid, make_module("ppo", ow, aw, STACK).to("cuda"))
        value = ppo.bind(aid, make_value_module(ow, STACK).to("cuda"))            # the parameters now live where the kernel reads them
        agents[aid] = dict(actor=actor, value=value, obs=o, act=a, actor_opt=torch.optim.Adam(actor.parameters(), lr=3e-4),
                           critic_opt=torch.optim.Adam(value.parameters(), lr=6e-4))
    # the reference stores the clamped delta, not the absolute action (PPO_org.py:284, 307): outputs["raw"]
    roll = env.capture(lambda obs: actors.act(buf.stacked_obs()),
                       on_step=lambda obs, rew: (buf.push(actors.actions), store.record(actors.outputs["raw"].double(), None)))
    env.reset()
    buf.begin()
    store.begin()
    for _ in range(steps):
        if roll.step():
            break
    rows = store.finish()
    old_log_probs = ppo.evaluate_store(store)                       # one launch: values[0 .. rows] are in the store, row `rows` the bootstrap value
    adv, td_target = store.compute_gae(GAMMA, LMBDA, normalize=True)
    v = store.views()
    # every state of every row as [rows * n_envs, STACK, n_obs] for the epochs (the kernel needed no such tensor)
    times = (torch.arange(rows, device="cuda")[:, None] - (STACK - 1) + torch.arange(STACK, device="cuda")[None, :]).clamp_(min=0)
    states = v["obs"][times].transpose(1, 2).reshape(rows * n_envs, STACK, env.n_obs)
    last = None
    for _ in range(epochs):
        for i, (aid, g) in enumerate(agents.items()):
            x = states[:, :, g["obs"]]
            aw = g["act"].stop - g["act"].start
            actions = v["actions"][:, :, g["act"]].reshape(-1, aw).float()
            old = old_log_probs[:, :, g["act"]].reshape(-1, aw)
            advantage = adv[:, :, i].reshape(-1, 1)
            mu, std = g["actor"](x)
            log_ratio = (Normal(mu, std).log_prob(actions) - old).clamp(-20, 20)
            ratio = torch.exp(log_ratio)
            actor_loss = torch.mean(-torch.min(ratio * advantage, torch.clamp(ratio, 1 - CLIP_EPS, 1 + CLIP_EPS) * advantage))
            critic_loss = F.mse_loss(g["value"](x), td_target[:, :, i].reshape(-1, 1))
            g["actor_opt"].zero_grad()
            g["critic_opt"].zero_grad()
            actor_loss.backward()
            critic_loss.backward()
            torch.nn.utils.clip_grad_norm_(g["actor"].parameters(), max_norm=0.5)
            torch.nn.utils.clip_grad_norm_(g["value"].parameters(), max_norm=0.5)
            g["actor_opt"].step()                                     # in place, on the packs
            g["critic_opt"].step()
            last = (actor_loss.item(), critic_loss.item(), ratio.mean().item())
    torch.cuda.synchronize()
    print(f"{dataset} x {n_envs} envs, {len(agents)} agents: {rows} rows ({roll.replays} replayed steps), {epochs} epochs of the clipped loss")
    print(f"  values {tuple(v['values'].shape)}, old_log_probs {tuple(old_log_probs.shape)}: mean V {v['values'].mean().item():+.4f}, "
          f"mean old log-prob {old_log_probs.mean().item():+.4f}, mean td_target {td_target.mean().item():+.4f}")
    if last is not None:
        print(f"  last agent: actor loss {last[0]:+.5f}, critic loss {last[1]:.5f}, mean ratio {last[2]:.4f}")
    before = old_log_probs.clone()                                   # (the next launch writes the same tensor)
    again = ppo.evaluate_store(store)                                # the stepped modules are what it reads
    print(f"  after the epochs: mean |log-prob - old| {(again - before).abs().mean().item():.3e}")
    buf.close()
    store.close()
    env.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
