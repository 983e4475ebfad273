"""The reference's whole PPO update of its recurrent agents (rl/agents/PPO_org.py:518-629 with ``use_stacked_obs=False`` and the KL early
stop) on the device: a captured rollout of the LSTM actors fills a rollout store; behind the rows ONE launch evaluates the value LSTMs over
the states and the next states and the old log-probabilities (``evaluate_store``), one turns them into TD targets and GAE
(``compute_gae``), the advantages are normalised by the caller's torch line, and the clipped-loss epochs -- both forwards over every env's
whole sequence, back-propagation through time, ``clip_grad_norm_``, both Adam steps and the stop of every agent -- run as five launches per
epoch in place in the packs (``update_store``), captured as one graph and replayed.  No torch module takes part; modules bound to the packs
would see every step.

    python examples/ppo_lstm_full_update.py [dataset] [n_envs] [policy_steps] [epochs]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.lstm import make_actor_module, make_value_module  # noqa: E402
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402

MAX_DELTA, GAMMA, LMBDA = 2.5, 0.99, 0.95


def main():
    dataset = sys.argv[1] if len(sys.argv) > 1 else "nine_intersections"
    n_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 24
    epochs = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    np.random.seed(0)
    torch.manual_seed(0)
    env = VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3")
    actors = env.lstm_actors(delta_actions=True, max_delta=MAX_DELTA, seed=4)
    store = env.rollout_store(capacity=steps)
    ppo = env.lstm_ppo_targets(actors)
    for aid in env.possible_agents:                                  # reference-shaped initial parameters, copied into the packs
        o, a = env.obs_slices[aid], env.action_slices[aid]
        actors.load_state_dict(aid, make_actor_module(o.stop - o.start, a.stop - a.start).state_dict())
        ppo.load_state_dict(aid, make_value_module(o.stop - o.start).state_dict())
    roll = env.capture(lambda obs: actors.act(obs), on_step=lambda obs, rew: store.record(actors.outputs["raw"].double(), None))
    env.reset()
    store.begin()
    actors.reset_hidden()
    for _ in range(steps):
        if roll.step():
            break
    rows = store.finish()
    res = ppo.evaluate_store(store)
    old_log_probs = res["old_log_probs"].clone()                     # (the next evaluate_store writes the same tensor)
    adv, td_target = ppo.compute_gae(store, res["values"], res["next_values"], GAMMA, LMBDA)
    adv = ((adv - adv.mean(dim=(0, 1))) / (adv.std(dim=(0, 1)) + 1e-8)).contiguous()      # the reference's normalisation line, per agent
    td_target = td_target.clone()
    ppo.update_store(store, old_log_probs, adv, td_target, epochs=epochs)      # eager once: allocates the workspace and the outputs
    torch.cuda.synchronize()
    first = dict(steps=ppo.adam_steps(), kl=ppo.epoch_outputs.approx_kl.tolist(), flags=ppo.epoch_outputs.stop_flags.tolist())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                       # begin_update and `epochs` x five launches: one chain
        ppo.update_store(store, old_log_probs, adv, td_target, epochs=epochs)
    graph.replay()                                                   # a second update of the same rollout, from the stepped parameters
    torch.cuda.synchronize()
    out = ppo.epoch_outputs
    print(f"{dataset} x {n_envs} envs, {len(env.possible_agents)} recurrent agents: {rows} rows ({roll.replays} replayed steps), two updates of "
          f"{epochs} epochs, the second replayed from a captured graph; workspace {ppo.update_workspace_bytes(rows, n_envs) / 2 ** 20:.1f} MiB")
    print(f"  first update: steps {first['steps']}, last approx_kl {[f'{v:+.2e}' for v in first['kl']]}, stopped {first['flags']}")
    print(f"  second update: steps {ppo.adam_steps()}, last approx_kl {[f'{v:+.2e}' for v in out.approx_kl.tolist()]}, stopped {out.stop_flags.tolist()}")
    print(f"  actor loss {[f'{v:+.5f}' for v in out.actor_loss.tolist()]}, critic loss {[f'{v:.5f}' for v in out.critic_loss.tolist()]}, "
          f"gradient norms {[f'{v:.3f}' for v in out.actor_norm.tolist()]} / {[f'{v:.3f}' for v in out.value_norm.tolist()]}")
    again = ppo.evaluate_store(store)["old_log_probs"]               # the stepped packs are what it reads
    print(f"  after the updates: mean |log-prob - old| {(again - old_log_probs).abs().mean().item():.3e}")
    ok = bool(torch.isfinite(again).all()) and max(ppo.adam_steps()) >= 1
    store.close()
    env.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
