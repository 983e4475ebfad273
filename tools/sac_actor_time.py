#!/usr/bin/env python3
"""What does the actor half of a SAC update cost per update (the actor's forward, the squashed sample, both online critics on it, the actor
loss, its backward pass, the actor's Adam step, the temperature loss and its Adam step, for every agent), and what does the whole update
cost with that half on the device, replayed as a captured graph?

    python tools/sac_actor_time.py [--out profiles/sac_actor_time.txt] [--datasets 45_intersections nine_intersections] [--batches 64 1024]
    python tools/sac_actor_time.py --setup DATASET B [--trace]                 one setup, its lines (what the driver runs)

  (a)   reference-shaped torch modules per agent (rl/agents/SAC.py:347-370 line by line), ONE fused capturable Adam over every actor and
        one over every log_alpha: the least torch can launch.  It uses nothing this repository did not have before the actor kernels
  (b)   SacTargets.actor_update: two launches
  (c)   the whole update sample -> td_target -> critic_update -> actor_update -> soft_update, all on the device
  (c')  the same with the actor half as in (a), on modules bound to the packs the kernels read and write

All are captured once on a filled replay store and replayed ALTERNATELY in one process, --reps times each, --replays replays per
repetition between two device events, behind a warm-up.  The spread between the repetitions of a case is the resolution of the
comparison.  The driver runs every setup as a process of its own under its own `timeout`, chained with `&&` (a step that fails or hangs
ends the chain), and (b) once more per setup under `rocprofv3 --kernel-trace --stats` for the kernels' own durations."""
import argparse
import glob
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK, MAX_DELTA, N_ENVS, LR = 5, 2.5, 256, 3e-4


def run_setup(dataset, B, reps, replays, trace):
    import torch
    from torch.distributions import Normal

    sys.path.insert(0, ROOT)
    from pednstream_amd.policy import make_module
    from pednstream_amd.rl_env import VecPedNetEnv
    from pednstream_amd.sac import make_critic_module

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
    s = buf.sample(B)[0].clone()
    torch.manual_seed(0)
    shapes = {aid: (env.obs_slices[aid].stop - env.obs_slices[aid].start, env.action_slices[aid].stop - env.action_slices[aid].start) for aid in agents}

    def modules():
        torch.manual_seed(1)
        return {aid: dict(actor=make_module("sac", *shapes[aid], STACK).cuda(), critics=[make_critic_module(*shapes[aid], STACK).cuda() for _ in range(4)],
                          log_alpha=torch.tensor(-4.6, device="cuda", requires_grad=True)) for aid in agents}

    def torch_half(nets, states):
        """the reference's lines 347-370 for every agent, and the two optimisers"""
        for aid in agents:
            for m in nets[aid]["critics"]:
                for p in m.parameters():
                    p.requires_grad_(False)                        # (the actor loss reads the critics; their step is not this half's)
        opt = torch.optim.Adam([p for aid in agents for p in nets[aid]["actor"].parameters()], lr=LR, capturable=True, fused=True)
        opt_alpha = torch.optim.Adam([nets[aid]["log_alpha"] for aid in agents], lr=LR, capturable=True, fused=True)

        def fn(x_all=None):
            x_all = states if x_all is None else x_all
            opt.zero_grad(set_to_none=True)
            opt_alpha.zero_grad(set_to_none=True)
            for aid in agents:
                n = nets[aid]
                x = x_all[:, :, env.obs_slices[aid]]
                mu, std = n["actor"](x)
                dist = Normal(mu, std, validate_args=False)      # (the validation reads the device: not capturable)
                u = dist.rsample()
                logp = dist.log_prob(u)
                new = torch.tanh(u)
                logp = logp - torch.log(1 - torch.tanh(new).pow(2) + 1e-7)
                new = new * MAX_DELTA
                entropy = -logp.sum(dim=1, keepdim=True)
                q = torch.min(n["critics"][0](x, new), n["critics"][1](x, new))
                torch.mean(-n["log_alpha"].exp().detach() * entropy - q).backward()
                torch.mean((entropy + float(shapes[aid][1])).detach() * n["log_alpha"].exp()).backward()
            opt.step()
            opt_alpha.step()

        return fn

    def device(nets, bind):
        actors = env.stacked_actors(kind="sac", stack_size=STACK, delta_actions=True, max_delta=MAX_DELTA, seed=1)
        sac = env.sac_targets(actors, seed=2)
        for aid in agents:
            n = nets[aid]
            if bind:
                actors.bind(aid, n["actor"])
                sac.bind(aid, *n["critics"], log_alpha=n["log_alpha"])
            else:
                actors.load_state_dict(aid, n["actor"].state_dict())
                for which, m in zip(("critic_1", "critic_2", "target_critic_1", "target_critic_2"), n["critics"]):
                    sac.load_state_dict(aid, which, m.state_dict())
        return sac

    from pednstream_amd import sac as sac_module

    cases = {}
    if not trace:
        cases["a"] = torch_half(modules(), s)
    if hasattr(sac_module.SacTargets, "actor_update"):             # (older commits: the baseline alone)
        sac_b = device(modules(), False)
        cases["b"] = lambda: sac_b.actor_update(s, actor_lr=LR, alpha_lr=LR)
        if not trace:
            sac_c = device(modules(), False)
            nets_d = modules()
            sac_d = device(nets_d, True)
            half_d = torch_half(nets_d, None)

            def whole(sac, actor_half):
                st, a, r, ns, d, _ = buf.sample(B)
                td = sac.td_target(r, ns, d)
                sac.critic_update(st, a.to(torch.float32), td, lr=LR)
                actor_half(st)
                sac.soft_update()

            cases["c"] = lambda: whole(sac_c, lambda st: sac_c.actor_update(st, actor_lr=LR, alpha_lr=LR))
            cases["c'"] = lambda: whole(sac_d, half_d)
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
    label = {"a": f"(a)   torch actor half, {len(agents)} agents, ONE Adam(capturable, fused) each for actors and log_alphas", "b": "(b)   actor_update",
             "c": "(c)   whole update, all on the device", "c'": "(c')  whole update, the actor half in torch"}
    for name, ts in times.items():
        print(f"{dataset} B {B:5d} {label[name]}: {min(ts):9.2f} us per update, best of {len(ts)} x {n} replays; all: "
              + " ".join(f"{t:.2f}" for t in ts) + f"; spread {max(ts) - min(ts):.2f}", flush=True)
    env.close()


def kernel_stats(trace_dir):
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "sacactor_" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs=2, metavar=("DATASET", "B"))
    ap.add_argument("--trace", action="store_true", help="(b) alone, a few replays: the run rocprofv3 wraps")
    ap.add_argument("--datasets", nargs="+", default=["45_intersections", "nine_intersections"])
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_actor_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "sac_actor_trace"))
    args = ap.parse_args()
    if args.setup:
        run_setup(args.setup[0], int(args.setup[1]), args.reps, args.replays, args.trace)
        return 0
    out = shlex.quote(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/sac_actor_time.py: the actor half of a SAC update for every agent (forward, sample, both critics, actor loss, backward, Adam; "
                f"temperature loss, Adam) and the whole update, one captured graph per case, replayed alternately ({args.reps} x {args.replays} "
                "replays each, device events)\n")
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
