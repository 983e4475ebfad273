#!/usr/bin/env python3
"""What does the gradient-free half of a SAC update cost per update (the TD targets of a sampled minibatch for every agent, then the
Polyak update of every target critic), replayed as a captured graph?

    python tools/sac_target_time.py [--out profiles/sac_target_time.txt] [--datasets 45_intersections nine_intersections] [--batches 64 1024]
    python tools/sac_target_time.py --setup DATASET B [--trace]                 one setup, its lines (what the driver runs)

  (a) the same computation with reference-shaped torch modules, per agent: the actor on its columns of the next stacks, mu + std * randn,
      tanh, the log-probability with the reference's second tanh, both target critics, their minimum, the entropy term, td_target; then
      the reference's soft_update line per parameter tensor of both target critics.  It uses nothing this repository did not have
      before the SAC kernels, so it runs unchanged on older commits: the baseline
  (b) SacTargets.td_target + SacTargets.soft_update: two launches

Both are captured once on the same sampled minibatch of a filled replay store and replayed ALTERNATELY in one process, --reps times each,
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
STACK, MAX_DELTA, GAMMA, TAU, N_ENVS = 5, 2.5, 0.99, 0.005, 256


def torch_nets(torch, obs_w, act_w):
    nn = torch.nn

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc = nn.Linear(STACK * obs_w, 64), nn.Linear(64, 64), nn.Linear(64, 64)
            self.fc_mu, self.fc_std = nn.Linear(64, act_w), nn.Linear(64, act_w)

        def forward(self, x):
            h = torch.relu(self.fc(torch.relu(self.fc2(torch.relu(self.fc1(x.transpose(1, 2).flatten(1)))))))
            return self.fc_mu(h), nn.functional.softplus(self.fc_std(h))

    class Critic(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc, self.fc_out = nn.Linear(STACK * obs_w, 64), nn.Linear(64, 64), nn.Linear(64 + act_w + 1, 64), nn.Linear(64, 1)

        def forward(self, s, a):
            zs = torch.relu(self.fc2(torch.relu(self.fc1(s.transpose(1, 2).flatten(1)))))
            return self.fc_out(self.fc(torch.cat([zs, a, s[:, -1, -1].unsqueeze(1)], dim=1)))

    make = lambda cls: cls().to("cuda").requires_grad_(False)
    return make(Actor), [make(Critic) for _ in range(4)]           # critic_1, critic_2, target_critic_1, target_critic_2


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
    _, _, r, ns, d, _ = buf.sample(B)
    torch.manual_seed(0)
    shapes = {aid: (env.obs_slices[aid].stop - env.obs_slices[aid].start, env.action_slices[aid].stop - env.action_slices[aid].start) for aid in agents}
    nets = {aid: torch_nets(torch, *shapes[aid]) for aid in agents}
    log_alpha = torch.full((len(agents),), -4.6051702, device="cuda")
    td_a = torch.zeros(B, len(agents), device="cuda")

    def case_a():
        for i, aid in enumerate(agents):
            actor, (c1, c2, t1, t2) = nets[aid]
            x = ns[:, :, env.obs_slices[aid]]
            mu, std = actor(x)
            u = mu + std * torch.randn(mu.shape, device="cuda")
            logp = -((u - mu) ** 2) / (2 * std ** 2) - std.log() - 0.9189385332046727
            na = torch.tanh(u)
            logp = logp - torch.log(1 - torch.tanh(na).pow(2) + 1e-7)
            na = na * MAX_DELTA
            entropy = -logp.sum(dim=1, keepdim=True)
            nv = torch.min(t1(x, na), t2(x, na)) + log_alpha[i].exp() * entropy
            td_a[:, i:i + 1] = r[:, i:i + 1] + GAMMA * nv * (1 - d.view(-1, 1))
        for aid in agents:
            _, (c1, c2, t1, t2) = nets[aid]
            for net, target in ((c1, t1), (c2, t2)):
                for pt, p in zip(target.parameters(), net.parameters()):
                    pt.data.copy_(pt.data * (1.0 - TAU) + p.data * TAU)

    cases = {"a": case_a}
    has_kernels = hasattr(env, "sac_targets")                      # (older commits: the baseline alone)
    if has_kernels:
        actors = env.stacked_actors(kind="sac", stack_size=STACK, delta_actions=True, max_delta=MAX_DELTA, seed=1)
        sac = env.sac_targets(actors, gamma=GAMMA, tau=TAU, seed=2)
        for aid in agents:
            actor, crit = nets[aid]
            actors.load_state_dict(aid, ref_keys(actor.state_dict()))
            for which, m in zip(("critic_1", "critic_2", "target_critic_1", "target_critic_2"), crit):
                sac.load_state_dict(aid, which, ref_keys(m.state_dict()))

        def case_b():
            sac.td_target(r, ns, d)
            sac.soft_update()

        cases["b"] = case_b
    if trace:
        cases = {"b": cases["b"]}
    graphs = {}
    for name, fn in cases.items():
        fn()                                                       # allocates
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        graphs[name] = g
    if has_kernels and not trace:                                  # the two compute the same thing (other noise, other summation order)
        torch.cuda.synchronize()
        gap = (td_a - sac.outputs["td_target"]).abs().mean().item()
        scale = td_a.abs().mean().item()
    times = {name: [] for name in graphs}
    for name, g in graphs.items():
        for _ in range(200):                                       # warm-up
            g.replay()
    for _ in range(1 if trace else reps):
        for name, g in graphs.items():                             # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(300 if trace else replays):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / (300 if trace else replays))
    label = {"a": f"(a) torch modules, {len(agents)} agents, per-tensor Polyak", "b": "(b) td_target + soft_update"}
    for name, ts in times.items():
        print(f"{dataset} B {B:5d} {label[name]}: {min(ts):8.2f} us per update, best of {len(ts)} x {replays} replays; all: "
              + " ".join(f"{t:.2f}" for t in ts) + f"; spread {max(ts) - min(ts):.2f}", flush=True)
    if has_kernels and not trace:
        print(f"{dataset} B {B:5d} mean |td_target (a) - (b)| {gap:.3e} at mean |td_target| {scale:.3e} (independent noise)", flush=True)
    env.close()


def kernel_stats(trace_dir):
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "sac_" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs=2, metavar=("DATASET", "B"))
    ap.add_argument("--trace", action="store_true", help="(b) alone, a few replays: the run rocprofv3 wraps")
    ap.add_argument("--datasets", nargs="+", default=["45_intersections", "nine_intersections"])
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_target_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "sac_target_trace"))
    args = ap.parse_args()
    if args.setup:
        run_setup(args.setup[0], int(args.setup[1]), args.reps, args.replays, args.trace)
        return 0
    out = shlex.quote(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/sac_target_time.py: SAC TD targets of a sampled minibatch for every agent + Polyak update of every target critic, one "
                f"captured graph per case, replayed alternately ({args.reps} x {args.replays} replays each, device events)\n")
    rc = 0
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --reps {args.reps} --replays {args.replays}"
    for dataset in args.datasets:
        for B in args.batches:
            trace = os.path.join(args.trace_dir, f"{dataset}_{B}")
            steps = [f"timeout -k 10 200 {me} --setup {shlex.quote(dataset)} {B} >> {out}",
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
