#!/usr/bin/env python3
"""What does the running normalisation cost in a graph-replayed rollout (45_intersections x 2048 envs, the 3-layer MLP of
tools/graph_rollout_time.py, one policy step per replay)?

    python tools/norm_time.py [--out profiles/norm_time.txt] [--envs 2048]      the whole measurement
    python tools/norm_time.py --case a|b|c [--envs N]                            one case, one line (what the driver runs)

  (a) no normalisation
  (b) the same contract written as torch ops inside policy_fn / on_step (running mean / variance of the tracked columns in float64,
      clip, discounted returns and their statistics) -- uses nothing this repository did not have before set_running_norm, so it runs
      unchanged on older commits: the baseline
  (c) VecPedNetEnv.set_running_norm(norm_obs=True, norm_reward=True)

The driver runs every GPU step as a process of its own under its own `timeout`, the steps chained with `&&` (a step that fails or hangs
ends the chain): (a) three times -- the spread between them is the resolution of the comparison --, (b), (c), and (c) once more under
`rocprofv3 --kernel-trace --stats` for the normalisation kernel's own duration."""
import argparse
import glob
import os
import shlex
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(case, B, calls_max=600):
    import torch

    sys.path.insert(0, ROOT)
    from pednstream_amd.rl_env import VecPedNetEnv

    env = VecPedNetEnv("45_intersections", n_envs=B, obs_mode="option3", action_gap=1, seed=0, data_dir=os.path.join(ROOT, "data"), history="recent")
    low = torch.as_tensor(env.action_low, device="cuda", dtype=torch.float64)
    span = torch.as_tensor(env.action_high, device="cuda", dtype=torch.float64) - low
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(env.n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                              torch.nn.Linear(64, env.n_actions), torch.nn.Sigmoid()).to("cuda").requires_grad_(False)
    total = torch.zeros(B, device="cuda")
    act = lambda x: (low + span * mlp(x).double()).contiguous()
    if case == "b":
        f = env.features_per_link
        n_agents = len(env.possible_agents)
        tracked = torch.ones(env.n_obs, dtype=torch.bool)
        for aid, ty in zip(env.possible_agents, env._types):
            if ty == 1:
                sl = env.obs_slices[aid]
                tracked[sl.start + f - 1:sl.stop:f] = False
        cols = torch.nonzero(tracked).reshape(-1).to("cuda")
        mean = torch.zeros(len(cols), device="cuda", dtype=torch.float64)
        var, count = torch.ones_like(mean), torch.full_like(mean, 1e-4)
        ret = torch.zeros((B, n_agents), device="cuda", dtype=torch.float64)
        rstat = torch.tensor([0.0, 1.0, 1e-4], device="cuda", dtype=torch.float64)
        normed = torch.zeros((B, env.n_obs), device="cuda")
        rew_n = torch.zeros((B, n_agents), device="cuda")

        def merge(m, v, c, bm, bv):
            delta = bm - m
            tot = c + B
            m2 = v * c + bv * B + delta * delta * c * B / tot
            return m + delta * B / tot, m2 / tot, tot

        def policy(obs):
            x = obs[:, cols].double()
            m, v, c = merge(mean, var, count, x.mean(dim=0), x.var(dim=0, unbiased=False))
            mean.copy_(m), var.copy_(v), count.copy_(c)
            normed.copy_(obs)
            normed[:, cols] = ((x - mean) / torch.sqrt(var + 1e-8)).clamp(-50.0, 50.0).float()
            return act(normed)

        def on_step(obs, rew):
            r = rew.double()
            ret.mul_(0.99).add_(r)
            for a in range(n_agents):          # agent after agent, like the reference's loop
                col = ret[:, a]
                m, v, c = merge(rstat[0], rstat[1], rstat[2], col.mean(), col.var(unbiased=False))
                rstat[0], rstat[1], rstat[2] = m, v, c
                rew_n[:, a] = (r[:, a] / torch.sqrt(rstat[1] + 1e-8)).clamp(-10.0, 10.0).float()
            total.add_(rew_n[:, 0])
    else:
        if case == "c":
            env.set_running_norm(norm_obs=True, norm_reward=True)
        policy = act
        on_step = lambda o, r: total.add_(r[:, 0])
    env.reset(seed=3)
    roll = env.capture(policy, on_step)
    for _ in range(4):
        roll.step()
    torch.cuda.synchronize()
    s0, calls = env.sim_step, 0
    t0 = time.perf_counter()
    while env.sim_step + 1 <= env.simulation_steps - 2 and calls < calls_max:
        roll.step()
        calls += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = env.sim_step - s0
    label = {"a": "(a) no normalisation", "b": "(b) the contract as torch ops in policy_fn / on_step", "c": "(c) set_running_norm"}[case]
    print(f"{label}: {B} envs, {dt / steps * 1e6:7.2f} us per replayed policy step ({steps} steps, replays {roll.replays}, eager {roll.eager_steps}, "
          f"recaptures {roll.recaptures})", flush=True)
    env.close()


def kernel_stats(trace_dir):
    """Lines of rocprofv3's kernel statistics that name the normalisation kernel (and the two step kernels next to it)."""
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "norm_kernel" in l or "link_turn_kernel" in l or "node_kernel" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["a", "b", "c"])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "norm_trace"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.envs)
        return 0
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --envs {args.envs}"
    out = shlex.quote(args.out)
    steps = [f"timeout -k 10 150 {me} --case {c} >> {out}" for c in ("a", "a", "a", "b", "c")]
    steps.append(f"timeout -k 10 240 rocprofv3 --kernel-trace --stats -d {shlex.quote(args.trace_dir)} -- {me} --case c > /dev/null")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/norm_time.py: graph-replayed MLP rollout, one policy step per replay\n")
    rc = subprocess.call(["bash", "-c", " && ".join(steps)])
    with open(args.out, "a") as f:
        if rc != 0:
            f.write(f"a step ended with status {rc}: the chain stopped there\n")
        else:
            f.write("kernel durations inside the replayed graph of (c), rocprofv3 --kernel-trace --stats (ns):\n")
            f.write("\n".join(kernel_stats(args.trace_dir)) + "\n")
    print(open(args.out).read())
    return rc


if __name__ == "__main__":
    sys.exit(main())
