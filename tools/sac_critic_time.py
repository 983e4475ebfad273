#!/usr/bin/env python3
"""What does the critic step of a SAC update cost per update (both critic forwards of every agent on a sampled minibatch, the two MSE
losses against the TD targets, their backward passes and one Adam step of every online critic), replayed as a captured graph?

    python tools/sac_critic_time.py [--out profiles/sac_critic_time.txt] [--datasets 45_intersections nine_intersections] [--batches 64 1024]
    python tools/sac_critic_time.py --setup DATASET B [--trace]                 one setup, its lines (what the driver runs)

  (a)  reference-shaped torch modules, per agent: critic_1 and critic_2 on the agent's columns, mse_loss against its column of td_target,
       backward, and one torch.optim.Adam(capturable=True) per critic as the reference has them.  It uses nothing this repository did not
       have before the critic kernels, so it runs unchanged on older commits: the baseline
  (a') the same with fused=True;  (a'') the same losses with ONE fused Adam over every critic of every agent: the least torch can launch
  (b)  SacTargets.critic_update: two launches

All are captured once on the same sampled minibatch of a filled replay store and replayed ALTERNATELY in one process, --reps times each,
--replays replays per repetition between two device events, behind a warm-up.  The spread between the repetitions of a case is the
resolution of the comparison.  The driver runs every setup as a process of its own under its own `timeout`, chained with `&&` (a step
that fails or hangs ends the chain), and (b) once more per setup under `rocprofv3 --kernel-trace --stats` for the kernels' own durations."""
import argparse
import glob
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK, MAX_DELTA, N_ENVS, LR = 5, 2.5, 256, 3e-4


def torch_critic(torch, obs_w, act_w):
    nn = torch.nn

    class Critic(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc, self.fc_out = nn.Linear(STACK * obs_w, 64), nn.Linear(64, 64), nn.Linear(64 + act_w + 1, 64), nn.Linear(64, 1)

        def forward(self, s, a):
            zs = torch.relu(self.fc2(torch.relu(self.fc1(s.transpose(1, 2).flatten(1)))))
            return self.fc_out(self.fc(torch.cat([zs, a, s[:, -1, -1].unsqueeze(1)], dim=1)))

    return Critic().to("cuda")


def ref_keys(sd):
    return {("encoder." + k if k[:3] in ("fc1", "fc2") else k): v for k, v in sd.items()}


def run_setup(dataset, B, reps, replays, trace):
    import torch

    sys.path.insert(0, ROOT)
    from pednstream_amd.rl_env import VecPedNetEnv

    env = VecPedNetEnv(dataset, n_envs=N_ENVS, obs_mode="option3", action_gap=1, seed=0, data_dir=os.path.join(ROOT, "data"), history="recent")
    agents = list(env.possible_agents)
    low, high = torch.as_tensor(env.action_low, device="cuda"), torch.as_tensor(env.action_high, device="cuda")
    const = (low + 0.5 * (high - low)).double().expand(N_ENVS, -1).contiguous()
    buf = env.replay_store(16, stack_size=STACK, seed=0)
    env.reset(seed=3)
    buf.begin()
    for _ in range(24):                                            # a filled store
        env.step_device(const, sync=True)
        buf.push(const)
    s, a, r, _, _, _ = buf.sample(B)
    torch.manual_seed(0)
    acts = (torch.rand(B, env.n_actions, device="cuda") * 2 - 1) * MAX_DELTA
    td = r + torch.randn(B, len(agents), device="cuda")
    shapes = {aid: (env.obs_slices[aid].stop - env.obs_slices[aid].start, env.action_slices[aid].stop - env.action_slices[aid].start) for aid in agents}
    start = {aid: [torch_critic(torch, *shapes[aid]) for _ in range(2)] for aid in agents}

    def torch_case(per_critic, fused):
        nets = {aid: [torch_critic(torch, *shapes[aid]) for _ in range(2)] for aid in agents}
        for aid in agents:
            for m, m0 in zip(nets[aid], start[aid]):
                m.load_state_dict(m0.state_dict())
        kw = dict(lr=LR, capturable=True, **({"fused": True} if fused else {}))
        if per_critic:
            opts = [torch.optim.Adam(m.parameters(), **kw) for aid in agents for m in nets[aid]]
        else:
            opts = [torch.optim.Adam([p for aid in agents for m in nets[aid] for p in m.parameters()], **kw)]

        def fn():
            for o in opts:
                o.zero_grad(set_to_none=True)
            for i, aid in enumerate(agents):
                x, ac, target = s[:, :, env.obs_slices[aid]], acts[:, env.action_slices[aid]], td[:, i:i + 1]
                for m in nets[aid]:
                    torch.nn.functional.mse_loss(m(x, ac), target).backward()
            for o in opts:
                o.step()

        return fn, nets

    cases, kept = {}, {}
    if not trace:
        for name, (per_critic, fused) in (("a", (True, False)), ("a'", (True, True)), ("a''", (False, True))):
            cases[name], kept[name] = torch_case(per_critic, fused)
    from pednstream_amd import sac as sac_module

    has_kernels = hasattr(sac_module.SacTargets, "critic_update")
    if has_kernels:                                                # (older commits: the baselines alone)
        actors = env.stacked_actors(kind="sac", stack_size=STACK, delta_actions=True, max_delta=MAX_DELTA, seed=1)
        sac = env.sac_targets(actors, seed=2)
        for aid in agents:
            for which, m in zip(("critic_1", "critic_2"), start[aid]):
                sac.load_state_dict(aid, which, ref_keys(m.state_dict()))
        cases["b"] = lambda: sac.critic_update(s, acts, td, lr=LR)
    graphs = {}
    for name, fn in cases.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):                                     # allocates; the optimisers' state comes to life
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        graphs[name] = g
    gap = None
    if has_kernels and not trace:                                  # the same step: 3 eager ones each so far, up to the order of the sums
        torch.cuda.synchronize()
        aid = agents[-1]
        mine = sac.parameters(aid, "critic_2")["fc.weight"]
        gap = ((mine - kept["a"][aid][1].fc.weight).abs().max().item(), (mine - start[aid][1].fc.weight).abs().max().item())
    times = {name: [] for name in graphs}
    for name, g in graphs.items():
        for _ in range(30):                                        # warm-up
            g.replay()
    n = 100 if trace else replays
    for _ in range(1 if trace else reps):
        for name, g in graphs.items():                             # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / n)
    label = {"a": f"(a)   torch, {len(agents)} agents, Adam(capturable) per critic", "a'": "(a')  torch, Adam(capturable, fused) per critic",
             "a''": "(a'') torch, ONE Adam(capturable, fused)", "b": "(b)   critic_update"}
    for name, ts in times.items():
        print(f"{dataset} B {B:5d} {label[name]}: {min(ts):9.2f} us per update, best of {len(ts)} x {n} replays; all: "
              + " ".join(f"{t:.2f}" for t in ts) + f"; spread {max(ts) - min(ts):.2f}", flush=True)
    if gap is not None:
        print(f"{dataset} B {B:5d} max |critic_2.fc.weight (a) - (b)| of the last agent behind 3 steps {gap[0]:.3e}; the 3 steps moved it by {gap[1]:.3e}", flush=True)
    env.close()


def kernel_stats(trace_dir):
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "critic_" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs=2, metavar=("DATASET", "B"))
    ap.add_argument("--trace", action="store_true", help="(b) alone, a few replays: the run rocprofv3 wraps")
    ap.add_argument("--datasets", nargs="+", default=["45_intersections", "nine_intersections"])
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_critic_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "sac_critic_trace"))
    args = ap.parse_args()
    if args.setup:
        run_setup(args.setup[0], int(args.setup[1]), args.reps, args.replays, args.trace)
        return 0
    out = shlex.quote(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/sac_critic_time.py: the critic step of a SAC update for every agent (forwards, MSE losses, backward, Adam), one captured "
                f"graph per case, replayed alternately ({args.reps} x {args.replays} replays each, device events)\n")
    rc = 0
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --reps {args.reps} --replays {args.replays}"
    for dataset in args.datasets:
        for B in args.batches:
            trace = os.path.join(args.trace_dir, f"{dataset}_{B}")
            steps = [f"timeout -k 10 240 {me} --setup {shlex.quote(dataset)} {B} >> {out}",
                     f"timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d {shlex.quote(trace)} -- {me} --setup {shlex.quote(dataset)} {B} --trace > /dev/null"]
            rc = subprocess.call(["bash", "-c", " && ".join(steps)])
            with open(args.out, "a") as f:
                if rc != 0:
                    f.write(f"a step ended with status {rc}: the chain stopped there\n")
                else:
                    f.write(f"kernel durations of (b) on {dataset}, B {B}, rocprofv3 --kernel-trace --stats (ns):\n")
                    f.write("\n".join(kernel_stats(trace)) + "\n")
            if rc != 0:
                break
        if rc != 0:
            break
    print(open(args.out).read())
    return rc


if __name__ == "__main__":
    sys.exit(main())
