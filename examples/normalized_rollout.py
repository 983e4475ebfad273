"""A graph-replayed MLP rollout on NORMALISED observations: 45_intersections x 2048 envs, the running statistics of the reference's
RunningNormalizeWrapper kept and updated on the device for the whole batch (VecPedNetEnv.set_running_norm).

    python examples/normalized_rollout.py [n_envs] [episodes]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402


def main():
    n_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    episodes = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    env = VecPedNetEnv("45_intersections", n_envs=n_envs, obs_mode="option3", history="recent")
    env.set_running_norm(norm_obs=True, norm_reward=True, clip_obs=50.0, clip_reward=10.0, gamma=0.99)
    low = torch.as_tensor(env.action_low, device="cuda", dtype=torch.float64)
    span = torch.as_tensor(env.action_high, device="cuda", dtype=torch.float64) - low
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(env.n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                              torch.nn.Linear(64, env.n_actions), torch.nn.Sigmoid()).to("cuda").requires_grad_(False)
    returns = torch.zeros(n_envs, device="cuda")            # of the normalised rewards
    true_returns = torch.zeros(n_envs, device="cuda")       # of the raw ones: raw_views() aliases the un-normalised buffers
    raw_rew = env.raw_views()[1]

    def policy(obs):                                        # obs: the normalised observation buffer
        return (low + span * mlp(obs).double()).contiguous()

    def on_step(obs, rew):
        returns.add_(rew[:, 0])
        true_returns.add_(raw_rew[:, 0])

    roll = env.capture(policy, on_step)
    for ep in range(episodes):
        env.reset(options={"randomize": True, "mode": "vectorised"}, seed=ep)
        returns.zero_(), true_returns.zero_()
        t0 = time.perf_counter()
        steps = 0
        while not roll.step():
            steps += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        stats = env.get_normalization_stats()
        first = env.possible_agents[0]
        print(f"episode {ep}: {dt / (steps + 1) * 1e6:.1f} us per policy step, mean return {true_returns.mean().item():.1f} "
              f"(normalised {returns.mean().item():.2f}); {first}: count {stats['obs_rms'][first]['count']:.0f}, "
              f"return std {stats['ret_rms']['var'] ** 0.5:.2f}; replays {roll.replays}, recaptures {roll.recaptures}")
    env.set_training(False)                                 # evaluation: the statistics are frozen, rows are still normalised
    env.close()


if __name__ == "__main__":
    main()
