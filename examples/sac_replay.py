"""Off-policy training data on the device: the loop of the reference's train_off_policy_multi_agent (rl/agents/SAC.py:127-225) for a whole
batch of envs.  The policy decides on the stack of the last four observations (``ReplayStore.stacked_obs``), every policy step is pushed
into the replay ring by a launch captured with the step, and after every step each agent draws a minibatch of stacked transitions
(``ReplayStore.sample``) for a small SAC-style update of this example's own (one Q network and a Gaussian actor per agent; not the
reference's networks, checkpoints or plots).

    python examples/sac_replay.py [dataset] [n_envs] [policy_steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402

STACK, BATCH, MINIMAL_SIZE, GAMMA, TAU, ALPHA = 4, 64, 500, 0.98, 0.005, 0.01


def mlp(n_in, n_out):
    return torch.nn.Sequential(torch.nn.Linear(n_in, 64), torch.nn.ReLU(), torch.nn.Linear(64, n_out)).to("cuda")


class Agent:
    def __init__(self, obs_dim, act_dim, low, high):
        self.actor, self.q, self.q_target = mlp(STACK * obs_dim, 2 * act_dim), mlp(STACK * obs_dim + act_dim, 1), mlp(STACK * obs_dim + act_dim, 1)
        self.q_target.load_state_dict(self.q.state_dict())
        self.low, self.span = low, high - low
        self.opt_actor = torch.optim.Adam(self.actor.parameters(), lr=3e-4)
        self.opt_q = torch.optim.Adam(self.q.parameters(), lr=3e-3)

    def act(self, stack, noise=None):
        """Actions in the agent's physical bounds and their log-density (up to a constant) from a stack [B, STACK, obs_dim]."""
        mean, log_std = self.actor(stack.flatten(1)).chunk(2, dim=1)
        log_std = log_std.clamp(-5.0, 1.0)
        u = mean + log_std.exp() * (torch.randn_like(mean) if noise is None else noise)
        a = torch.sigmoid(u)
        logp = (-0.5 * ((u - mean) / log_std.exp()) ** 2 - log_std - torch.log(a * (1 - a) + 1e-6)).sum(1)
        return self.low + self.span * a, logp

    def update(self, s, a, r, ns, d):
        a = a.float()
        with torch.no_grad():
            na, nlogp = self.act(ns)
            target = r + GAMMA * (1 - d) * (self.q_target(torch.cat([ns.flatten(1), na], 1)).squeeze(1) - ALPHA * nlogp)
        q_loss = torch.nn.functional.mse_loss(self.q(torch.cat([s.flatten(1), a], 1)).squeeze(1), target)
        self.opt_q.zero_grad()
        q_loss.backward()
        self.opt_q.step()
        pa, logp = self.act(s)
        actor_loss = (ALPHA * logp - self.q(torch.cat([s.flatten(1), pa], 1)).squeeze(1)).mean()
        self.opt_actor.zero_grad()
        actor_loss.backward()
        self.opt_actor.step()
        with torch.no_grad():
            for p, pt in zip(self.q.parameters(), self.q_target.parameters()):
                pt.mul_(1 - TAU).add_(TAU * p)
        return q_loss.detach()


def main():
    dataset = sys.argv[1] if len(sys.argv) > 1 else "nine_intersections"
    n_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    policy_steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    env = VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3")
    torch.manual_seed(0)
    low = torch.as_tensor(env.action_low, device="cuda")
    high = torch.as_tensor(env.action_high, device="cuda")
    agents = {aid: Agent(env.obs_slices[aid].stop - env.obs_slices[aid].start, env.action_slices[aid].stop - env.action_slices[aid].start,
                         low[env.action_slices[aid]], high[env.action_slices[aid]]) for aid in env.possible_agents}
    episode = env.simulation_steps // env.action_gap
    buf = env.replay_store(capacity=2 * episode, stack_size=STACK, seed=0)
    kept = {}

    def policy(obs):                                    # the state is the stack, not the single frame the env hands over
        stack = buf.stacked_obs()
        with torch.no_grad():
            kept["actions"] = torch.cat([agents[aid].act(stack[:, :, env.obs_slices[aid]])[0] for aid in env.possible_agents], 1).double().contiguous()
        return kept["actions"]

    roll = env.capture(policy, on_step=lambda obs, rew: buf.push(kept["actions"]))
    steps = updates = 0
    losses = torch.zeros(len(agents), device="cuda")
    while steps < policy_steps:
        env.reset()
        buf.begin()
        done = False
        while not done and steps < policy_steps:
            done = roll.step()
            steps += 1
            if steps * n_envs > MINIMAL_SIZE:           # the host's own count: no look at the device
                for i, (aid, agent) in enumerate(agents.items()):
                    s, a, r, ns, d, _ = buf.sample(BATCH, agent=aid)
                    losses[i] = agent.update(s, a, r, ns, d)
                updates += 1
    s, a, r, ns, d, idx = buf.sample(BATCH, agent=env.possible_agents[0])
    print(f"{dataset} x {n_envs} envs: {steps} policy steps pushed ({roll.replays} replayed, {roll.eager_steps} eager), {buf.size()} transitions in a "
          f"ring of {buf.ring_slots} rows ({buf.nbytes / 2 ** 20:.1f} MiB), {updates} updates of {len(agents)} agents")
    print(f"  minibatch of {env.possible_agents[0]}: states {tuple(s.shape)}, actions {tuple(a.shape)} {str(a.dtype).replace('torch.', '')}, rewards "
          f"{tuple(r.shape)}, next_states {tuple(ns.shape)}, dones {tuple(d.shape)}, idx {tuple(idx.shape)}")
    print(f"  shared frames: next_states[:, :-1] == states[:, 1:] is {bool(torch.equal(ns[:, :-1], s[:, 1:]))}; last Q losses "
          + ", ".join(f"{x:.3e}" for x in losses.tolist()))
    buf.close()
    env.close()


if __name__ == "__main__":
    main()
