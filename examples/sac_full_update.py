"""The reference's whole SAC update (rl/agents/SAC.py:320-377) on the device, with no torch module in it: a captured rollout of the stacked
actors fills the replay store (examples/sac_actors.py); every few policy steps ONE captured graph samples a whole-row minibatch, computes
the TD targets of all agents (``td_target``), steps every online critic (``critic_update``), steps every actor and every temperature
(``actor_update``) and moves every target critic (``soft_update``).  The delta actions the critics see are formed by torch tensor
arithmetic inside the same graph.  examples/sac_critic_update.py is the same loop with the actor half in torch.

    python examples/sac_full_update.py [dataset] [n_envs] [policy_steps]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.policy import make_module  # noqa: E402
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402
from pednstream_amd.sac import make_critic_module  # noqa: E402

STACK, BATCH, MAX_DELTA = 5, 64, 2.5


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
    slices = []
    for aid in env.possible_agents:                                   # torch's initialisation of the reference's networks; no module is kept
        o, a = env.obs_slices[aid], env.action_slices[aid]
        ow, aw = o.stop - o.start, a.stop - a.start
        actors.load_state_dict(aid, make_module("sac", ow, aw, STACK).state_dict())
        c1, c2 = make_critic_module(ow, aw, STACK).state_dict(), make_critic_module(ow, aw, STACK).state_dict()
        for which, sd in (("critic_1", c1), ("critic_2", c2), ("target_critic_1", c1), ("target_critic_2", c2)):
            sac.load_state_dict(aid, which, sd)
        slices.append((o, a, aw))
    critic_actions = torch.zeros(BATCH, env.n_actions, dtype=torch.float32, device="cuda")

    def update(step=True):
        s, a, r, ns, d, _ = buf.sample(BATCH)                        # whole rows: every agent's columns of ONE draw
        td = sac.td_target(r, ns, d)                                  # [BATCH, n_agents]
        for o, ac, aw in slices:                                      # the delta actions that were taken: what the critics see
            width = s[:, -1, o].reshape(BATCH, aw, -1)[:, :, -1]
            critic_actions[:, ac] = (a[:, ac].float() - width).clamp(-MAX_DELTA, MAX_DELTA)
        if step:
            sac.critic_update(s, critic_actions, td, lr=3e-4)         # every online critic: two launches
            sac.actor_update(s, actor_lr=3e-4, alpha_lr=3e-4)         # every actor and log_alpha, through the stepped critics: two launches
        else:
            sac.critic_gradients(s, critic_actions, td)
            sac.actor_gradients(s)
        sac.soft_update()                                             # every target critic: one launch

    roll = env.capture(lambda obs: actors.act(buf.stacked_obs()), on_step=lambda obs, rew: buf.push(actors.actions))
    env.reset()
    buf.begin()
    graph, updates, start = None, 0, None
    for t in range(steps):
        roll.step()
        if t < 8 or t % 4:
            continue
        if graph is None:
            update(step=False)                                        # a warm call with the steps switched off: it allocates
            torch.cuda.synchronize()
            start = actors.parameters(env.possible_agents[0])["fc.weight"].clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                update()
        graph.replay()                                                # the whole update: the captured launches, nothing else
        updates += 1
    torch.cuda.synchronize()
    print(f"{dataset} x {n_envs} envs, {len(slices)} agents, {steps} policy steps ({roll.replays} replayed), {updates} updates of {BATCH} rows in one "
          f"captured graph: {sac.adam_steps()} critic steps and {sac.actor_adam_steps()} actor steps on the device, {sac.actor_draws()} actor launches drew noise")
    if updates:
        out = sac.actor_outputs
        moved = (actors.parameters(env.possible_agents[0])["fc.weight"] - start).abs().max().item()
        finite = bool(torch.isfinite(out.actor_loss).all() and torch.isfinite(sac.critic_outputs.losses).all() and torch.isfinite(sac.log_alpha).all())
        print(f"  last agent: critic losses {sac.critic_outputs.losses[-1][0].item():.4f} {sac.critic_outputs.losses[-1][1].item():.4f}, actor loss "
              f"{out.actor_loss[-1].item():.4f}, alpha loss {out.alpha_loss[-1].item():.4f}, log_alpha {sac.log_alpha[-1].item():.4f}; the first actor's "
              f"fc.weight moved by {moved:.2e}; the next act reads it; all finite: {finite}")
    buf.close()
    env.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
