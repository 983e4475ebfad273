"""Collect one PPO rollout on the device: a graph-replayed episode of a small actor / critic that fills a RolloutStore (one launch per
policy step, captured with the step), then the reference's TD targets, GAE and normalised advantages for every (env, agent) trajectory.
No training loop.

    python examples/ppo_rollout.py [dataset] [n_envs]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402


def main():
    dataset = sys.argv[1] if len(sys.argv) > 1 else "nine_intersections"
    n_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    env = VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3")
    n_agents = len(env.possible_agents)
    low = torch.as_tensor(env.action_low, device="cuda", dtype=torch.float64)
    span = torch.as_tensor(env.action_high, device="cuda", dtype=torch.float64) - low
    torch.manual_seed(0)
    body = lambda out, last: torch.nn.Sequential(torch.nn.Linear(env.n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, out), last).to("cuda").requires_grad_(False)
    actor, critic = body(env.n_actions, torch.nn.Sigmoid()), body(n_agents, torch.nn.Identity())
    store = env.rollout_store()                         # capacity: the policy steps of an episode
    kept = {}

    def policy(obs):                                    # the critic sees the state the action is decided in
        kept["actions"] = (low + span * actor(obs).double()).contiguous()
        kept["values"] = critic(obs).contiguous()
        return kept["actions"]

    roll = env.capture(policy, on_step=lambda obs, rew: store.record(kept["actions"], kept["values"]))
    env.reset()
    store.begin()
    while not roll.step():
        pass
    rows = store.finish()                               # the last row is terminated: no bootstrap value needed
    adv, td_target = store.compute_gae(0.99, 0.95, normalize=True)
    v = store.views()
    print(f"{dataset} x {n_envs} envs: {rows} rows (overflow {store.overflow}), replays {roll.replays}, eager steps {roll.eager_steps}")
    for k in ("obs", "actions", "values", "rewards", "done", "td_target", "advantages"):
        print(f"  {k:11s} {tuple(v[k].shape)} {str(v[k].dtype).replace('torch.', '')}")
    one = store.agent(env.possible_agents[0])
    print(f"  agent {env.possible_agents[0]}: obs {tuple(one['obs'].shape)}, actions {tuple(one['actions'].shape)}, advantages {tuple(one['advantages'].shape)}")
    print(f"  checksum: sum |advantages_raw| = {v['advantages_raw'].double().abs().sum().item():.6e}, normalised mean {adv.double().mean().item():+.2e}, "
          f"terminated rows {int(v['done'][:, 0].sum().item())}")
    env.close()


if __name__ == "__main__":
    main()
