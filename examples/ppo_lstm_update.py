"""The reference's PPO update with its default, recurrent agents (rl/agents/PPO_org.py:20-138, 518-629; use_stacked_obs=False) with the
gradient-free half on the device: a captured rollout of the stateful LSTM actors (``VecPedNetEnv.lstm_actors``, the hidden state lives on
the device) fills a rollout store; behind the rows ONE launch runs the value LSTM over the states and over the next states and the actor
LSTM with the old log-probabilities of the stored delta actions (``VecPedNetEnv.lstm_ppo_targets``); one more turns them into TD targets
and GAE.  The reference's normalisation line and one epoch of its clipped loss run in torch on modules whose parameters are bound to the
packs the kernels read; an env is a batch row of the modules.

    python examples/ppo_lstm_update.py [dataset] [n_envs] [policy_steps]
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Normal

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.lstm import make_actor_module, make_value_module  # noqa: E402
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402

MAX_DELTA, GAMMA, LMBDA, CLIP_EPS = 2.5, 0.99, 0.95, 0.2


def main():
    dataset = sys.argv[1] if len(sys.argv) > 1 else "nine_intersections"
    n_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    np.random.seed(0)
    torch.manual_seed(0)
    env = VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3")
    actors = env.lstm_actors(delta_actions=True, max_delta=MAX_DELTA, seed=4)
    store = env.rollout_store(capacity=steps)
    ppo = env.lstm_ppo_targets(actors)
    agents = {}
    for aid in env.possible_agents:
        o, a = env.obs_slices[aid], env.action_slices[aid]
        ow, aw = o.stop - o.start, a.stop - a.start
        actor = actors.bind(aid, make_actor_module(ow, aw).to("cuda"))
        value = ppo.bind(aid, make_value_module(ow).to("cuda"))                    # the parameters now live where the kernels read them
        agents[aid] = dict(actor=actor, value=value, obs=o, act=a, actor_opt=torch.optim.Adam(actor.parameters(), lr=3e-4),
                           critic_opt=torch.optim.Adam(value.parameters(), lr=6e-4))
    # the reference stores the clamped delta, not the absolute action (PPO_org.py:284, 307): outputs["raw"]
    roll = env.capture(lambda obs: actors.act(obs), on_step=lambda obs, rew: store.record(actors.outputs["raw"].double(), None))
    env.reset()
    store.begin()
    actors.reset_hidden()                                            # reset_buffer(): actor_hidden = None
    for _ in range(steps):
        if roll.step():
            break
    rows = store.finish()
    res = ppo.evaluate_store(store)                                  # one launch: three LSTM runs per agent, each from a zero state
    adv, td_target = ppo.compute_gae(store, res["values"], res["next_values"], GAMMA, LMBDA)
    old_log_probs = res["old_log_probs"]
    v = store.views()
    last = None
    for i, (aid, g) in enumerate(agents.items()):
        x = v["obs"][:rows, :, g["obs"]].transpose(0, 1)             # [n_envs, rows, obs_w]: an env is a batch row
        aw = g["act"].stop - g["act"].start
        actions = v["actions"][:, :, g["act"]].transpose(0, 1).float()
        old = old_log_probs[:, :, g["act"]].transpose(0, 1)
        advantage = adv[:, :, i].transpose(0, 1).unsqueeze(-1)
        advantage = (advantage - advantage.mean()) / (advantage.std() + 1e-8)      # the reference's normalisation line
        mu, std, _ = g["actor"](x)
        log_ratio = (Normal(mu, std).log_prob(actions) - old).clamp(-20, 20)
        ratio = torch.exp(log_ratio)
        actor_loss = torch.mean(-torch.min(ratio * advantage, torch.clamp(ratio, 1 - CLIP_EPS, 1 + CLIP_EPS) * advantage))
        values, _ = g["value"].forward_all_steps(x)
        critic_loss = F.mse_loss(values, td_target[:, :, i].transpose(0, 1).unsqueeze(-1))
        g["actor_opt"].zero_grad()
        g["critic_opt"].zero_grad()
        actor_loss.backward()
        critic_loss.backward()
        torch.nn.utils.clip_grad_norm_(g["actor"].parameters(), max_norm=0.5)
        torch.nn.utils.clip_grad_norm_(g["value"].parameters(), max_norm=0.5)
        g["actor_opt"].step()                                         # in place, on the packs
        g["critic_opt"].step()
        last = (actor_loss.item(), critic_loss.item(), ratio.mean().item())
    torch.cuda.synchronize()
    print(f"{dataset} x {n_envs} envs, {len(agents)} agents: {rows} rows ({roll.replays} replayed steps) of the LSTM actors, 1 epoch of the clipped loss")
    print(f"  values {tuple(res['values'].shape)}, next_values {tuple(res['next_values'].shape)}, old_log_probs {tuple(old_log_probs.shape)}: "
          f"mean V {res['values'].mean().item():+.4f}, mean old log-prob {old_log_probs.mean().item():+.4f}, mean td_target {td_target.mean().item():+.4f}")
    print(f"  last agent: actor loss {last[0]:+.5f}, critic loss {last[1]:.5f}, mean ratio {last[2]:.4f}")
    before = old_log_probs.clone()                                   # (the next launch writes the same tensor)
    again = ppo.evaluate_store(store)["old_log_probs"]               # the stepped modules are what it reads
    print(f"  after the epoch: mean |log-prob - old| {(again - before).abs().mean().item():.3e}")
    store.close()
    env.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
