#!/usr/bin/env python3
"""What does collecting a PPO rollout cost in a graph-replayed episode (45_intersections x 2048 envs, the 3-layer MLP of
tools/norm_time.py plus a critic head, one policy step per replay), and what does GAE over the episode cost?

    python tools/rollout_time.py [--out profiles/rollout_time.txt] [--envs 2048]     the whole measurement
    python tools/rollout_time.py --case a|b|c [--envs N]                              one case, one line (what the driver runs)

  (a) nothing stored (the critic still runs: the three cases replay the same policy kernels)
  (b) the transition stored with torch ops inside on_step (index_copy_ into preallocated [T, ...] tensors at a device-resident row
      counter), then TD targets with torch ops and GAE as a torch loop over the T time rows -- uses nothing this repository did not
      have before the rollout store, so it runs unchanged on older commits: the baseline
  (c) RolloutStore.record inside on_step, RolloutStore.compute_gae

The driver runs every GPU step as a process of its own under its own `timeout`, the steps chained with `&&` (a step that fails or hangs
ends the chain): (a), (b), (c), then (a) twice more -- the spread between the three is the resolution of the comparison --, and (c) once
more under `rocprofv3 --kernel-trace --stats` for the kernels' own durations."""
import argparse
import glob
import os
import shlex
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, LMBDA = 0.99, 0.95


def run_case(case, B):
    import torch

    sys.path.insert(0, ROOT)
    from pednstream_amd.rl_env import VecPedNetEnv

    env = VecPedNetEnv("45_intersections", n_envs=B, obs_mode="option3", action_gap=1, seed=0, data_dir=os.path.join(ROOT, "data"), history="recent")
    T, A = env.simulation_steps // env.action_gap, len(env.possible_agents)
    low = torch.as_tensor(env.action_low, device="cuda", dtype=torch.float64)
    span = torch.as_tensor(env.action_high, device="cuda", dtype=torch.float64) - low
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(env.n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                              torch.nn.Linear(64, env.n_actions), torch.nn.Sigmoid()).to("cuda").requires_grad_(False)
    critic = torch.nn.Sequential(torch.nn.Linear(env.n_obs, 64), torch.nn.Tanh(), torch.nn.Linear(64, A)).to("cuda").requires_grad_(False)
    total = torch.zeros(B, device="cuda")
    kept = {}

    def policy(obs):
        kept["a"] = (low + span * mlp(obs).double()).contiguous()
        kept["v"] = critic(obs).contiguous()
        return kept["a"]

    store = None
    if case == "b":
        row = torch.zeros(1, dtype=torch.int64, device="cuda")
        buf = {"actions": torch.zeros((T, B, env.n_actions), dtype=torch.float64, device="cuda"), "values": torch.zeros((T + 1, B, A), device="cuda"),
               "rewards": torch.zeros((T, B, A), device="cuda"), "done": torch.zeros((T, B, 1), device="cuda"),
               "obs": torch.zeros((T + 1, B, env.n_obs), device="cuda")}
        horizon = T - 1

        def on_step(obs, rew):
            buf["actions"].index_copy_(0, row, kept["a"].unsqueeze(0))
            buf["values"].index_copy_(0, row, kept["v"].unsqueeze(0))
            buf["rewards"].index_copy_(0, row, rew.unsqueeze(0))
            buf["done"].index_copy_(0, row, (row >= horizon).float().expand(B, 1).unsqueeze(0))
            buf["obs"].index_copy_(0, row + 1, obs.unsqueeze(0))
            row.add_(1)
            total.add_(rew[:, 0])
    elif case == "c":
        store = env.rollout_store()

        def on_step(obs, rew):
            store.record(kept["a"], kept["v"])
            total.add_(rew[:, 0])
    else:
        on_step = lambda o, r: total.add_(r[:, 0])
    roll = env.capture(policy, on_step)
    times = []
    for episode in range(3):                      # the first one captures
        env.reset(seed=3)
        if store is not None:
            store.begin()
        if case == "b":
            row.zero_()
            buf["obs"][0].copy_(env.device_views()[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while not roll.step():
            pass
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if case == "b":
            td_target = buf["rewards"] + GAMMA * buf["values"][1:] * (1 - buf["done"])
            delta = td_target - buf["values"][:-1]
            adv = torch.empty_like(delta)
            carry = torch.zeros_like(delta[0])
            c = torch.tensor(GAMMA * LMBDA, device="cuda")
            for t in range(T - 1, -1, -1):
                carry = c * carry + delta[t]
                adv[t] = carry
            flat = adv.reshape(-1, A)
            adv_n = (adv - flat.mean(dim=0)) / (flat.std(dim=0) + 1e-8)
            check = float(adv_n[0, 0, 0])
        elif case == "c":
            rows = store.finish()
            adv_n, _ = store.compute_gae(GAMMA, LMBDA, normalize=True)
            check = float(adv_n[0, 0, 0])
            assert rows == T and not store.overflow
        else:
            check = float(total[0])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        times.append((t1 - t0, t2 - t1))
    label = {"a": "(a) nothing stored", "b": "(b) stored with torch ops in on_step, GAE as a torch loop over T", "c": "(c) RolloutStore"}[case]
    ep, post = min(t[0] for t in times[1:]), min(t[1] for t in times[1:])
    print(f"{label}: {B} envs, {T} policy steps, {ep / T * 1e6:7.2f} us per policy step, {post * 1e3:8.3f} ms behind the episode (targets, GAE, "
          f"normalisation; check {check:+.6e}); replays {roll.replays}, eager {roll.eager_steps}, recaptures {roll.recaptures}", flush=True)
    env.close()


def kernel_stats(trace_dir):
    """Lines of rocprofv3's kernel statistics that name the rollout kernels (and the two step kernels next to them)."""
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "rollout_" in l or "link_turn_kernel" in l or "node_kernel" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["a", "b", "c"])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "rollout_trace"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.envs)
        return 0
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --envs {args.envs}"
    out = shlex.quote(args.out)
    steps = [f"timeout -k 10 150 {me} --case {c} >> {out}" for c in ("a", "b", "c", "a", "a")]
    steps.append(f"timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d {shlex.quote(args.trace_dir)} -- {me} --case c > /dev/null")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/rollout_time.py: graph-replayed MLP rollout of whole episodes, one policy step per replay\n")
    rc = subprocess.call(["bash", "-c", " && ".join(steps)])
    with open(args.out, "a") as f:
        if rc != 0:
            f.write(f"a step ended with status {rc}: the chain stopped there\n")
        else:
            f.write("kernel durations of (c), rocprofv3 --kernel-trace --stats (ns):\n")
            f.write("\n".join(kernel_stats(args.trace_dir)) + "\n")
    print(open(args.out).read())
    return rc


if __name__ == "__main__":
    sys.exit(main())
