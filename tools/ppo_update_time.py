#!/usr/bin/env python3
"""What does one epoch of PPO's clipped-loss update cost for every agent: (a) the torch epochs of examples/ppo_update.py on reference-shaped
modules with one fused capturable Adam per network kind, against (b) PpoTargets.epoch_update?

    python tools/ppo_update_time.py [--out profiles/ppo_update_time.txt]
    python tools/ppo_update_time.py --setup NAME T N [--groups G] [--only-b]        one setup, its lines (what the driver runs)

The tensors are SYNTHETIC, of the shapes of section 16's two setups (45_intersections: one agent of 20 observation columns and 4 actions,
700 rows; nine_intersections: three agents of 15, 20 and 15 columns and 3, 4 and 3 actions, 500 rows; 2048 envs, stacks of five) and of a
small one (nine_intersections' agents, 24 rows of 64 envs): what is computed does not depend on where the numbers came from, and no env has to
play an episode first.  (a) gets its [T * N, S, n_obs] tensor of stacks built outside the timed region and uses nothing of
pednstream_amd.ppo's epochs.  Both are captured as a graph and replayed ALTERNATELY in one process, --reps repetitions of --replays replays
between two device events behind a warm-up; the spread between the repetitions is the resolution.  The driver runs every setup as a process
of its own under its own `timeout`, chained with `&&`, then (b) at half and double the default number of groups, then (b) once more under
`rocprofv3 --kernel-trace --stats` for the kernels' own durations."""
import argparse
import glob
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK = 5
SETUPS = {"45_intersections": [(20, 4)], "nine_intersections": [(15, 3), (20, 4), (15, 3)]}


def run_setup(name, T, N, reps, replays, groups, only_b):
    import numpy as np
    import torch
    from torch.distributions import Normal

    sys.path.insert(0, ROOT)
    from pednstream_amd.policy import StackedActors, make_module
    from pednstream_amd.ppo import PpoTargets, make_value_module

    torch.manual_seed(0)
    widths = SETUPS[name]
    agents, o, a = [], 0, 0
    for ow, aw in widths:
        agents.append((o, ow, a, aw))
        o, a = o + ow, a + aw
    n_obs, n_actions = o, a
    sa = StackedActors("ppo", agents, np.zeros(n_actions, dtype=np.float32), np.full(n_actions, 4.0, dtype=np.float32), N, n_obs, n_actions,
                       stack_size=STACK, delta_actions=False)
    ppo = PpoTargets(sa)
    mods = []
    for i, (_, ow, _, aw) in enumerate(agents):
        am, vm = make_module("ppo", ow, aw, STACK).cuda(), make_value_module(ow, STACK).cuda()
        sa.load_state_dict(i, am.state_dict())
        ppo.load_state_dict(i, vm.state_dict())
        mods.append((am, vm))
    obs = torch.randn(T + 1, N, n_obs, device="cuda")
    ev = ppo.evaluate(obs, torch.zeros(T, N, n_actions, device="cuda"), want_mu_std=True)
    act = (ev["mu"] + ev["std"] * torch.randn(T, N, n_actions, device="cuda")).contiguous()          # samples of the policy
    old = (ppo.evaluate(obs, act)["old_log_probs"] + 0.1 * torch.randn(T, N, n_actions, device="cuda")).contiguous()
    adv, td = torch.randn(T, N, len(agents), device="cuda"), torch.randn(T, N, len(agents), device="cuda")
    head = f"{name} shapes ({len(agents)} agents), {T} x {N} rows"
    cases = {}
    if not only_b:
        times_idx = (torch.arange(T, device="cuda")[:, None] - (STACK - 1) + torch.arange(STACK, device="cuda")[None, :]).clamp_(min=0)
        states = obs[times_idx].transpose(1, 2).reshape(T * N, STACK, n_obs)
        print(f"{head} (a) needs a stacks tensor of {states.numel() * 4 / 2 ** 20:.1f} MiB", flush=True)
        xs = [states[:, :, o0:o0 + ow].contiguous() for (o0, ow, _, _) in agents]      # (an agent's columns, copied once outside the timed region)
        oa = torch.optim.Adam([p for am, _ in mods for p in am.parameters()], lr=3e-4, fused=True, capturable=True)
        ov = torch.optim.Adam([p for _, vm in mods for p in vm.parameters()], lr=6e-4, fused=True, capturable=True)

        def epoch_a():
            oa.zero_grad(set_to_none=False)
            ov.zero_grad(set_to_none=False)
            for i, ((o0, ow, a0, aw), (am, vm)) in enumerate(zip(agents, mods)):
                x = xs[i]
                mu, std = am(x)
                ratio = torch.exp((Normal(mu, std, validate_args=False).log_prob(act[:, :, a0:a0 + aw].reshape(-1, aw)) - old[:, :, a0:a0 + aw].reshape(-1, aw)).clamp(-20, 20))
                A = adv[:, :, i].reshape(-1, 1)
                torch.mean(-torch.min(ratio * A, torch.clamp(ratio, 0.8, 1.2) * A)).backward()
                torch.nn.functional.mse_loss(vm(x), td[:, :, i].reshape(-1, 1)).backward()
                torch.nn.utils.clip_grad_norm_(am.parameters(), max_norm=0.5)
                torch.nn.utils.clip_grad_norm_(vm.parameters(), max_norm=0.5)
            oa.step()
            ov.step()

        cases["a"] = epoch_a
    cases["b"] = lambda: ppo.epoch_update(obs, act, old, adv, td, kl_tolerance=float("inf"), groups=groups)
    graphs = {}
    side = torch.cuda.Stream()
    for key, fn in cases.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                              # warm-up on the side stream (allocates), then the capture
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        graphs[key] = g
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    times = {key: [] for key in graphs}
    for _ in range(reps):
        for key, g in graphs.items():                              # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[key].append(e0.elapsed_time(e1) / replays)
    ws = ppo._ulast["ws"]
    label = {"a": "(a) torch epochs, fused capturable Adam per kind", "b": f"(b) epoch_update, groups {groups or 'default'} ({ws.shape[0]} slabs, workspace {ws.numel() * 4 / 2 ** 20:.1f} MiB)"}
    for key, ts in times.items():
        print(f"{head} {label[key]}: {min(ts):9.3f} ms per epoch, best of {len(ts)} x {replays} replays; all: " + " ".join(f"{t:.3f}" for t in ts)
              + f"; spread {max(ts) - min(ts):.3f}", flush=True)


def kernel_stats(trace_dir):
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "ppograd" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs=3, metavar=("NAME", "T", "N"))
    ap.add_argument("--groups", type=int, default=None)
    ap.add_argument("--only-b", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "ppo_update_trace"))
    args = ap.parse_args()
    if args.setup:
        run_setup(args.setup[0], int(args.setup[1]), int(args.setup[2]), args.reps, args.replays, args.groups, args.only_b)
        return 0
    out = shlex.quote(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/ppo_update_time.py: one epoch of PPO's clipped-loss update for every agent on synthetic tensors of the setups' shapes, captured "
                f"and replayed alternately ({args.reps} repetitions behind a warm-up, device events)\n")
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --reps {args.reps}"
    trace = os.path.join(args.trace_dir, "nine_intersections")
    steps = [f"timeout -k 10 150 {me} --replays 3 --setup 45_intersections 700 2048 >> {out}",
             f"timeout -k 10 200 {me} --replays 3 --setup nine_intersections 500 2048 >> {out}",
             f"timeout -k 10 100 {me} --replays 50 --setup nine_intersections 24 64 >> {out}",
             f"timeout -k 10 100 {me} --replays 3 --only-b --groups 256 --setup nine_intersections 500 2048 >> {out}",
             f"timeout -k 10 100 {me} --replays 3 --only-b --groups 1024 --setup nine_intersections 500 2048 >> {out}",
             f"timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d {shlex.quote(trace)} -- {me} --replays 3 --only-b "
             f"--setup nine_intersections 500 2048 > /dev/null"]
    rc = subprocess.call(["bash", "-c", " && ".join(steps)])
    with open(args.out, "a") as f:
        if rc != 0:
            f.write(f"a step ended with status {rc}: the chain stopped there\n")
        else:
            f.write("kernel durations of (b) on nine_intersections' shapes, 500 x 2048 rows, rocprofv3 --kernel-trace --stats (ns):\n")
            f.write("\n".join(kernel_stats(trace)) + "\n")
    print(open(args.out).read())
    return rc


if __name__ == "__main__":
    sys.exit(main())
