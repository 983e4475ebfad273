#!/usr/bin/env python3
"""What does one epoch of PPO's clipped-loss update cost for every RECURRENT agent with LstmPpoTargets.epoch_update, and how does it split
over its five launches?

    python tools/lstm_update_time.py [--out profiles/lstm_update_time.txt]
    python tools/lstm_update_time.py --setup NAME T N [--groups G]        one setup, its line (what the driver runs)

The tensors are SYNTHETIC, of the shapes of section 17's setups (45_intersections: one agent of 20 observation columns and 4 actions, 700
rows; nine_intersections: three agents of 15, 20 and 15 columns and 3, 4 and 3 actions, 500 rows; 2048 envs) and of a small one
(nine_intersections' agents, 24 rows of 64 envs).  The epoch is captured as a graph and replayed, --reps repetitions of --replays replays
between two device events behind a warm-up; the spread between the repetitions is the resolution.  The driver runs every setup as a
process of its own under its own `timeout`, chained with `&&`, then both whole-episode setups once more under `rocprofv3 --kernel-trace
--stats` for the kernels' own durations.

There is NO torch side in this tool.  It had one -- the epochs of examples/ppo_lstm_update.py (nn.LSTM over every env's whole sequence,
autograd through time, one fused capturable Adam per network kind), captured and replayed alternately with the device epochs as
tools/ppo_update_time.py does -- and with it the 700 x 2048 setup ended with a segmentation fault of the process before its first line.
The cause was not found, so that path is taken out and the comparison against torch is not made."""
import argparse
import glob
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETUPS = {"45_intersections": [(20, 4)], "nine_intersections": [(15, 3), (20, 4), (15, 3)]}


def run_setup(name, T, N, reps, replays, groups):
    import faulthandler

    faulthandler.enable()                                          # a crash inside a library names the Python line it came from
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from pednstream_amd.lstm import LstmActors, LstmPpoTargets, make_actor_module, make_value_module

    torch.manual_seed(0)
    widths = SETUPS[name]
    agents, o, a = [], 0, 0
    for ow, aw in widths:
        agents.append((o, ow, a, aw))
        o, a = o + ow, a + aw
    n_obs, n_actions = o, a
    la = LstmActors(agents, np.zeros(n_actions, dtype=np.float32), np.full(n_actions, 4.0, dtype=np.float32), N, n_obs, n_actions, delta_actions=False)
    ppo = LstmPpoTargets(la)
    mods = []
    for i, (_, ow, _, aw) in enumerate(agents):
        am, vm = make_actor_module(ow, aw).cuda(), make_value_module(ow).cuda()
        la.load_state_dict(i, am.state_dict())
        ppo.load_state_dict(i, vm.state_dict())
        mods.append((am, vm))
    obs = torch.randn(T + 1, N, n_obs, device="cuda")
    ev = ppo.evaluate(obs, torch.zeros(T, N, n_actions, device="cuda"), want_mu_std=True)
    act = (ev["mu"] + ev["std"] * torch.randn(T, N, n_actions, device="cuda")).contiguous()          # samples of the policy
    old = (ppo.evaluate(obs, act)["old_log_probs"] + 0.1 * torch.randn(T, N, n_actions, device="cuda")).contiguous()
    adv, td = torch.randn(T, N, len(agents), device="cuda"), torch.randn(T, N, len(agents), device="cuda")
    head = f"{name} shapes ({len(agents)} agents), {T} x {N} rows"
    cases = {}
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
        for key, g in graphs.items():                            
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[key].append(e0.elapsed_time(e1) / replays)
    ws = ppo._ulast["ws"]
    label = {"b": f"epoch_update, groups {groups or 'default'} ({ws.shape[0]} slabs, workspace {ppo.update_workspace_bytes(T, N, groups) / 2 ** 20:.1f} MiB)"}
    for key, ts in times.items():
        print(f"{head} {label[key]}: {min(ts):9.3f} ms per epoch, best of {len(ts)} x {replays} replays; all: " + " ".join(f"{t:.3f}" for t in ts)
              + f"; spread {max(ts) - min(ts):.3f}", flush=True)


def kernel_stats(trace_dir):
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "lstmgrad" in l or "ppograd" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs=3, metavar=("NAME", "T", "N"))
    ap.add_argument("--groups", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_update_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "lstm_update_trace"))
    args = ap.parse_args()
    if args.setup:
        run_setup(args.setup[0], int(args.setup[1]), int(args.setup[2]), args.reps, args.replays, args.groups)
        return 0
    out = shlex.quote(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/lstm_update_time.py: one epoch of PPO's clipped-loss update for every recurrent agent on synthetic tensors of the setups' shapes, captured "
                f"and replayed ({args.reps} repetitions behind a warm-up, device events)\n")
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --reps {args.reps}"
    traces = {name: os.path.join(args.trace_dir, name) for name in ("45_intersections", "nine_intersections")}
    prof = "rocprofv3 --kernel-trace --stats --output-format csv -d"
    steps = [f"timeout -k 10 240 {me} --replays 3 --setup 45_intersections 700 2048 >> {out}",
             f"timeout -k 10 300 {me} --replays 3 --setup nine_intersections 500 2048 >> {out}",
             f"timeout -k 10 100 {me} --replays 50 --setup nine_intersections 24 64 >> {out}",
             f"timeout -k 10 200 {prof} {shlex.quote(traces['45_intersections'])} -- {me} --replays 3 --setup 45_intersections 700 2048 > /dev/null",
             f"timeout -k 10 200 {prof} {shlex.quote(traces['nine_intersections'])} -- {me} --replays 3 --setup nine_intersections 500 2048 > /dev/null"]
    rc = subprocess.call(["bash", "-c", " && ".join(steps)])
    with open(args.out, "a") as f:
        if rc != 0:
            f.write(f"a step ended with status {rc}: the chain stopped there\n")
        else:
            for name, rows in (("45_intersections", "700 x 2048"), ("nine_intersections", "500 x 2048")):
                f.write(f"kernel durations on {name}' shapes, {rows} rows, rocprofv3 --kernel-trace --stats (ns):\n")
                f.write("\n".join(kernel_stats(traces[name])) + "\n")
    print(open(args.out).read())
    return rc


if __name__ == "__main__":
    sys.exit(main())
