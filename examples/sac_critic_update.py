"""The reference's SAC update (rl/agents/SAC.py:320-377) with the TD targets, the CRITIC STEP and the Polyak update on the device: a captured
rollout of the stacked actors fills the replay store (examples/sac_actors.py); every few policy steps one launch computes the TD targets of
a whole-row minibatch for all agents, two launches compute q1, q2, both MSE losses, their gradients and one Adam step of every online
critic (``SacTargets.critic_update``), the actor and alpha losses and their Adam steps run in torch on modules whose parameters are bound to
the packs the kernels read and write (they see the stepped critics with no copy), and one launch does the Polyak update of every target
critic.  examples/sac_update.py is the same loop with the critic step in torch.

    python examples/sac_critic_update.py [dataset] [n_envs] [policy_steps]
"""
import os
import sys

import numpy as np
import torch
from torch.distributions import Normal

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.policy import make_module  # noqa: E402
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402
from pednstream_amd.sac import make_critic_module  # noqa: E402

STACK, BATCH, MAX_DELTA, TARGET_ENTROPY = 5, 64, 2.5, 0.0


def main():
    dataset = sys.argv[1] if len(sys.argv) > 1 else "nine_intersections"
    n_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    np.random.seed(0)
    torch.manual_seed(0)
    env = VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3")
    buf = env.replay_store(capacity=64, stack_size=STACK, seed=0)
    actors = env.stacked_actors(kind="sac", stack_size=STACK, delta_actions=True, max_delta=MAX_DELTA, seed=4)
    sac = env.sac_targets(actors, gamma=0.99, tau=0.005, seed=5)
    agents = {}
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        ow, aw = o.stop - o.start, a.stop - a.start
        actor = actors.bind(aid, make_module("sac", ow, aw, STACK).to("cuda"))
        c1, c2, t1, t2 = (make_critic_module(ow, aw, STACK).to("cuda") for _ in range(4))
        t1.load_state_dict(c1.state_dict())
        t2.load_state_dict(c2.state_dict())
        log_alpha = torch.tensor(np.log(0.01), dtype=torch.float32, device="cuda", requires_grad=True)
        sac.bind(aid, c1, c2, t1, t2, log_alpha=log_alpha)          # the parameters and log_alpha now live where the kernels read them
        for p in list(c1.parameters()) + list(c2.parameters()):
            p.requires_grad_(False)                                   # the device trains the critics; the actor's loss only reads them
        agents[aid] = dict(actor=actor, c1=c1, c2=c2, log_alpha=log_alpha, obs=o, act=a,
                           opt=torch.optim.Adam([{"params": actor.parameters()}, {"params": [log_alpha]}], lr=3e-4))
    critic_actions = torch.zeros(BATCH, env.n_actions, dtype=torch.float32, device="cuda")
    roll = env.capture(lambda obs: actors.act(buf.stacked_obs()), on_step=lambda obs, rew: buf.push(actors.actions))
    env.reset()
    buf.begin()
    updates, last = 0, None
    for t in range(steps):
        roll.step()
        if t < 8 or t % 4:
            continue
        s, a, r, ns, d, _ = buf.sample(BATCH)                        # whole rows: every agent's columns of ONE draw
        td = sac.td_target(r, ns, d)                                  # [BATCH, n_agents]: one launch, nothing to detach
        for g in agents.values():                                     # the delta actions that were taken: what the critics see
            width = s[:, -1, g["obs"]].reshape(BATCH, g["act"].stop - g["act"].start, -1)[:, :, -1]
            critic_actions[:, g["act"]] = (a[:, g["act"]].float() - width).clamp(-MAX_DELTA, MAX_DELTA)
        sac.critic_update(s, critic_actions, td, lr=3e-4)             # every online critic of every agent: two launches
        for aid, g in agents.items():
            x = s[:, :, g["obs"]]
            mu, std = g["actor"](x)
            u = Normal(mu, std).rsample()
            new = torch.tanh(u)
            logp = Normal(mu, std).log_prob(u) - torch.log(1 - torch.tanh(new).pow(2) + 1e-7)
            entropy = -logp.sum(dim=1, keepdim=True)
            new = new * MAX_DELTA
            q = torch.min(g["c1"](x, new), g["c2"](x, new))           # the stepped critics, read in place
            actor_loss = (-g["log_alpha"].exp().detach() * entropy - q).mean()
            alpha_loss = ((entropy - TARGET_ENTROPY).detach() * g["log_alpha"].exp()).mean()
            g["opt"].zero_grad()
            (actor_loss + alpha_loss).backward()
            g["opt"].step()                                           # in place, on the packs
            last = (aid, actor_loss.item(), g["log_alpha"].item())
        sac.soft_update()                                             # every target critic of every agent: one launch
        updates += 1
    torch.cuda.synchronize()
    print(f"{dataset} x {n_envs} envs, {len(agents)} agents, {steps} policy steps ({roll.replays} replayed), {updates} updates of {BATCH} rows: "
          f"{sac.adam_steps()} critic steps on the device, {sac.draws()} target launches drew noise")
    if last is not None:
        losses = sac.critic_outputs.losses[-1]
        print(f"  last agent: critic losses {losses[0].item():.4f} {losses[1].item():.4f}, actor loss {last[1]:.4f}, log_alpha {last[2]:.4f}; "
              f"td_target mean {sac.outputs['td_target'].mean().item():.4f}, losses finite: {bool(torch.isfinite(sac.critic_outputs.losses).all())}")
    buf.close()
    env.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
