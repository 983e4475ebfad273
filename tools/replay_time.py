#!/usr/bin/env python3
"""What does feeding an off-policy trainer cost in a graph-replayed episode (45_intersections x 2048 envs, the 3-layer MLP of
tools/rollout_time.py on the stack of the last four observations, one policy step per replay)?

    python tools/replay_time.py [--out profiles/replay_time.txt] [--envs 2048]     the whole measurement
    python tools/replay_time.py --case a|b|c|d|s [--envs N]                         one case, one line (what the driver runs)

  (a) nothing stored: the MLP reads a [n_envs, 4, n_obs] tensor that nobody updates (the same policy kernels as the other cases)
  (b) the same ring written with torch ops inside on_step -- an index_copy_ per array at a device-resident head, the stack rolled with
      torch ops, and per agent one minibatch of 64: torch.randint / torch.rand indices, the clamp rule as index arithmetic, advanced-
      indexing gathers.  It uses nothing this repository did not have before the replay store, so it runs unchanged on older commits:
      the baseline
  (c) ReplayStore.push plus one ReplayStore.sample(64) per agent inside on_step
  (d) ReplayStore.push alone
  (s) ReplayStore.sample on a filled store, 200 calls each of B = 64 and B = 4096, whole rows and one agent's columns

The capacity is the largest whose store stays under 4 GB.  The driver runs every GPU step as a process of its own under its own
`timeout`, the steps chained with `&&` (a step that fails or hangs ends the chain): (a), (b), (c), (d), (a), (a) -- the spread between the
three (a) runs is the resolution of the comparison --, (s), and (c) once more under `rocprofv3 --kernel-trace --stats` for the kernels'
own durations."""
import argparse
import glob
import os
import shlex
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK, BATCH, LIMIT = 4, 64, 4_000_000_000


def largest_capacity(env, episode):
    from pednstream_amd.replay import ring_slots

    row = env.n_envs * (env.n_obs * 4 + env.n_actions * 8 + len(env.possible_agents) * 4) + 12
    fixed = env.n_envs * STACK * env.n_obs * 4 + 64
    cap = (LIMIT - fixed) // (row + 8)
    while ring_slots(cap, STACK, episode) * row + cap * 8 + fixed >= LIMIT:
        cap -= 1
    return cap


def run_case(case, B):
    import torch

    sys.path.insert(0, ROOT)
    from pednstream_amd.rl_env import VecPedNetEnv

    env = VecPedNetEnv("45_intersections", n_envs=B, obs_mode="option3", action_gap=1, seed=0, data_dir=os.path.join(ROOT, "data"), history="recent")
    T, A, O = env.simulation_steps // env.action_gap, len(env.possible_agents), env.n_obs
    agents = list(env.possible_agents)
    low = torch.as_tensor(env.action_low, device="cuda", dtype=torch.float64)
    span = torch.as_tensor(env.action_high, device="cuda", dtype=torch.float64) - low
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(STACK * O, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                              torch.nn.Linear(64, env.n_actions), torch.nn.Sigmoid()).to("cuda").requires_grad_(False)
    total = torch.zeros(B, device="cuda")
    kept = {}
    cap = largest_capacity(env, T)
    buf = env.replay_store(cap, stack_size=STACK, seed=0) if case in "cds" else None
    stack = torch.zeros(B, STACK, O, device="cuda") if buf is None else None

    def policy(obs):
        # (the MLP runs, its output is weighted with 0: every case applies the same actions, so the step kernels, whose time depends on
        # how busy the corridors are, are not driven apart by what the stack happens to hold)
        kept["a"] = (low + span * (0.5 + 0.0 * mlp((stack if buf is None else buf.stacked_obs()).flatten(1)).double())).contiguous()
        return kept["a"]

    if case == "b":
        from pednstream_amd.replay import ring_slots

        R = ring_slots(cap, STACK, T)
        ring = {"frames": torch.zeros((R, B, O), device="cuda"), "actions": torch.zeros((R, B, env.n_actions), dtype=torch.float64, device="cuda"),
                "rewards": torch.zeros((R, B, A), device="cuda"), "done": torch.zeros((R, 1), device="cuda"),
                "first": torch.zeros((R, 1), dtype=torch.int64, device="cuda")}
        head, first = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
        back = torch.arange(STACK, -1, -1, device="cuda").view(1, -1)
        sink = torch.zeros((), device="cuda")

        def torch_begin():
            ring["frames"].index_copy_(0, head % R, env.device_views()[0].unsqueeze(0))
            ring["first"].index_copy_(0, head % R, torch.full((1, 1), -1, dtype=torch.int64, device="cuda"))
            first.copy_(head)
            head.add_(1)
            stack.copy_(env.device_views()[0].unsqueeze(1).expand(-1, STACK, -1))

        def on_step(obs, rew):
            slot = head % R
            ring["frames"].index_copy_(0, slot, obs.unsqueeze(0))
            ring["actions"].index_copy_(0, slot, kept["a"].unsqueeze(0))
            ring["rewards"].index_copy_(0, slot, rew.unsqueeze(0))
            ring["done"].index_copy_(0, slot, (head - first >= T).float().view(1, 1))
            ring["first"].index_copy_(0, slot, first.view(1, 1))
            head.add_(1)
            stack.copy_(torch.cat([stack[:, 1:], obs.unsqueeze(1)], 1))
            size = (head - 1 - first).clamp(max=cap)
            for i, aid in enumerate(agents):          # (drawn from the running episode alone: no RESET row to step over)
                rank = (torch.rand(BATCH, device="cuda") * size).long()
                env_i = torch.randint(0, B, (BATCH,), device="cuda")
                serial = head - 1 - rank
                rows = serial % R
                q = ring["first"][rows, 0]
                frames = torch.maximum(serial.view(-1, 1) - back, q.view(-1, 1)) % R          # [BATCH, STACK + 1]
                x = ring["frames"][frames, env_i.view(-1, 1), env.obs_slices[aid]]
                s, ns = x[:, :STACK], x[:, 1:]
                a = ring["actions"][rows, env_i, env.action_slices[aid]]
                r = ring["rewards"][rows, env_i, i]
                d = ring["done"][rows, 0]
                sink.add_(s.sum() + ns.sum() + a.sum().float() + r.sum() + d.sum())          # (the minibatch is consumed)
            total.add_(rew[:, 0])
    elif case == "c":
        def on_step(obs, rew):
            buf.push(kept["a"])
            for aid in agents:
                buf.sample(BATCH, agent=aid)
            total.add_(rew[:, 0])
    elif case in "ds":
        def on_step(obs, rew):
            buf.push(kept["a"])
            total.add_(rew[:, 0])
    else:
        on_step = lambda o, r: total.add_(r[:, 0])
    roll = env.capture(policy, on_step)
    times = []
    for episode in range(2 if case == "s" else 3):                      # the first one captures
        env.reset(seed=3)
        if buf is not None:
            buf.begin()
        elif case == "b":
            torch_begin()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while not roll.step():
            pass
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    ep = min(times[1:])
    what = f"replays {roll.replays}, eager {roll.eager_steps}, recaptures {roll.recaptures}"
    if case == "s":
        for batch in (64, 4096):
            for aid in (None, agents[0]):
                buf.sample(batch, agent=aid)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(200):
                    out = buf.sample(batch, agent=aid)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / 200
                moved = sum(t.numel() * t.element_size() for t in out)
                print(f"(s) sample({batch}, agent={aid}): {dt * 1e6:7.2f} us per call back to back, {moved / 1e6:.3f} MB written per call "
                      f"(states {tuple(out[0].shape)})", flush=True)
        per_transition = B * (2 * STACK * O * 4 + env.n_actions * 8 + A * 4 + 4)
        print(f"(s) capacity {cap} rows x {B} envs = {cap * B} transitions of {A} agents in {buf.nbytes / 1e9:.3f} GB (ring of {buf.ring_slots} rows, "
              f"n_obs {O}); a stack-per-transition layout ({2 * STACK} copies of every observation) would take {cap * per_transition / 1e9:.3f} GB; "
              f"size_rows {buf.size_rows()}", flush=True)
    else:
        label = {"a": "(a) nothing stored", "b": f"(b) ring, stack and {A} minibatches of {BATCH} with torch ops in on_step",
                 "c": f"(c) ReplayStore.push + {A} x sample({BATCH}) in on_step", "d": "(d) ReplayStore.push alone"}[case]
        print(f"{label}: {B} envs, {T} policy steps, {ep / T * 1e6:7.2f} us per policy step (check {float(total[0]):+.6e}); {what}", flush=True)
    env.close()


def kernel_stats(trace_dir):
    """Lines of rocprofv3's kernel statistics that name the replay kernels (and the two step kernels next to them)."""
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "replay_" in l or "link_turn_kernel" in l or "node_kernel" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["a", "b", "c", "d", "s"])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "replay_trace"))
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.envs)
        return 0
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --envs {args.envs}"
    out = shlex.quote(args.out)
    steps = [f"timeout -k 10 150 {me} --case {c} >> {out}" for c in ("a", "b", "c", "d", "a", "a", "s")]
    steps.append(f"timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d {shlex.quote(args.trace_dir)} -- {me} --case c > /dev/null")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/replay_time.py: graph-replayed MLP rollout of whole episodes on the stacked observation, one policy step per replay\n")
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
