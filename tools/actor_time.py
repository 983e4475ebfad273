#!/usr/bin/env python3
"""What does the decision cost in a graph-replayed episode (2048 envs, the reference's stacked SAC actor per agent on the stack of the
last five observations, one policy step per replay, every step pushed into a replay store)?

    python tools/actor_time.py [--out profiles/actor_time.txt] [--envs 2048] [--datasets 45_intersections nine_intersections]
    python tools/actor_time.py --case a|b|c --dataset NAME [--envs N]              one case, one line (what the driver runs)

  (a) the same-shape actors as torch modules inside the captured policy: per agent the forward on its slice of the stack, noise from a
      registered generator, tanh * max_delta, the delta on the newest frame's gate widths, the clip, and one cat + .double() for the
      row.  It uses nothing this repository did not have before the actor kernel, so it runs unchanged on older commits: the baseline
  (b) StackedActors.act(buf.stacked_obs()): one launch
  (c) a constant action tensor: the floor

Every case applies the same constant actions (the policy's output enters with weight 0 through one torch.add), so the step kernels,
whose time depends on how busy the corridors are, are not driven apart; (b) - (c) therefore includes that one torch.add.  The driver
runs every GPU step as a process of its own under its own `timeout`, the steps chained with `&&` (a step that fails or hangs ends the
chain): (a), (b), (c), (c), (c) -- the spread between the three (c) runs is the resolution of the comparison --, and (b) once more
under `rocprofv3 --kernel-trace --stats` for the kernel's own duration.  Best of the two episodes behind the capturing one."""
import argparse
import glob
import os
import shlex
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK, MAX_DELTA = 5, 2.5


def torch_actor(torch, obs_w, act_w):
    nn = torch.nn

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc = nn.Linear(STACK * obs_w, 64), nn.Linear(64, 64), nn.Linear(64, 64)
            self.fc_mu, self.fc_std = nn.Linear(64, act_w), nn.Linear(64, act_w)

        def forward(self, x):
            h = torch.relu(self.fc(torch.relu(self.fc2(torch.relu(self.fc1(x.transpose(1, 2).flatten(1)))))))
            return self.fc_mu(h), nn.functional.softplus(self.fc_std(h))

    return Actor().to("cuda").requires_grad_(False)


def run_case(case, dataset, B):
    import torch

    sys.path.insert(0, ROOT)
    from pednstream_amd.rl_env import VecPedNetEnv

    env = VecPedNetEnv(dataset, n_envs=B, obs_mode="option3", action_gap=1, seed=0, data_dir=os.path.join(ROOT, "data"), history="recent")
    T, agents = env.simulation_steps // env.action_gap, list(env.possible_agents)
    low = torch.as_tensor(env.action_low, device="cuda")
    high = torch.as_tensor(env.action_high, device="cuda")
    const = (low + 0.5 * (high - low)).double().expand(B, -1).contiguous()
    torch.manual_seed(0)
    shapes = {aid: (env.obs_slices[aid].stop - env.obs_slices[aid].start, env.action_slices[aid].stop - env.action_slices[aid].start) for aid in agents}
    mods = {aid: torch_actor(torch, *shapes[aid]) for aid in agents}
    buf = env.replay_store(8, stack_size=STACK, seed=0)
    total = torch.zeros(B, device="cuda")
    applied = torch.zeros(B, env.n_actions, dtype=torch.float64, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    if case == "a":
        def policy(obs):
            stack, rows = buf.stacked_obs(), []
            for aid in agents:
                o, a = env.obs_slices[aid], env.action_slices[aid]
                x = stack[:, :, o]
                mu, std = mods[aid](x)
                raw = torch.tanh(mu + std * torch.randn(mu.shape, generator=gen, device="cuda")) * MAX_DELTA
                width = x[:, -1].view(B, shapes[aid][1], -1)[:, :, -1]
                rows.append(torch.maximum(torch.minimum(width + raw, high[a]), low[a]))
            return torch.add(const, torch.cat(rows, 1).double(), alpha=0.0, out=applied)
    elif case == "b":
        actors = env.stacked_actors(kind="sac", stack_size=STACK, delta_actions=True, max_delta=MAX_DELTA, seed=1)
        for aid in agents:
            sd = mods[aid].state_dict()
            actors.load_state_dict(aid, {("encoder." + k if k[:3] in ("fc1", "fc2") else k): v for k, v in sd.items()})

        def policy(obs):
            return torch.add(const, actors.act(buf.stacked_obs()), alpha=0.0, out=applied)
    else:
        policy = lambda obs: const

    def on_step(obs, rew):
        buf.push(const if case == "c" else applied)
        total.add_(rew[:, 0])

    roll = env.capture(policy, on_step, generators=(gen,) if case == "a" else ())
    times = []
    for episode in range(3):                      # the first one captures
        env.reset(seed=3)
        buf.begin()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while not roll.step():
            pass
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    ep = min(times[1:])
    label = {"a": f"(a) {len(agents)} torch actors in the captured policy", "b": "(b) StackedActors.act", "c": "(c) constant actions"}[case]
    print(f"{dataset} {label}: {B} envs, {len(agents)} agents, n_obs {env.n_obs}, n_actions {env.n_actions}, {T} policy steps, "
          f"{ep / T * 1e6:8.2f} us per policy step (check {float(total[0]):+.6e}); replays {roll.replays}, eager {roll.eager_steps}, "
          f"recaptures {roll.recaptures}", flush=True)
    env.close()


def kernel_stats(trace_dir):
    """Lines of rocprofv3's kernel statistics that name the actor kernel (and the step and push kernels next to it)."""
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "actor_" in l or "replay_push" in l or "link_turn_kernel" in l or "node_kernel" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["a", "b", "c"])
    ap.add_argument("--dataset")
    ap.add_argument("--datasets", nargs="+", default=["45_intersections", "nine_intersections"])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_time.txt"))
    ap.add_argument("--append", action="store_true", help="keep what the file holds (a second call for another dataset)")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "actor_trace"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.dataset or args.datasets[0], args.envs)
        return 0
    out = shlex.quote(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if not args.append:
        with open(args.out, "w") as f:
            f.write("tools/actor_time.py: graph-replayed rollout of whole episodes, the stacked SAC actors on the last five observations, one "
                    "policy step per replay\n")
    rc = 0
    for dataset in args.datasets:
        me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --envs {args.envs} --dataset {shlex.quote(dataset)}"
        trace = os.path.join(args.trace_dir, dataset)
        steps = [f"timeout -k 10 150 {me} --case {c} >> {out}" for c in ("a", "b", "c", "c", "c")]
        steps.append(f"timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d {shlex.quote(trace)} -- {me} --case b > /dev/null")
        rc = subprocess.call(["bash", "-c", " && ".join(steps)])
        with open(args.out, "a") as f:
            if rc != 0:
                f.write(f"a step ended with status {rc}: the chain stopped there\n")
            else:
                f.write(f"kernel durations of (b) on {dataset}, rocprofv3 --kernel-trace --stats (ns):\n")
                f.write("\n".join(kernel_stats(trace)) + "\n")
        if rc != 0:
            break
    print(open(args.out).read())
    return rc


if __name__ == "__main__":
    sys.exit(main())
