#!/usr/bin/env python3
"""What does the gradient-free half of a PPO update cost behind an episode: the value of every state, and the old log-probabilities of
the actions, for every agent, env and row of a filled rollout store?

    python tools/ppo_eval_time.py [--out profiles/ppo_eval_time.txt] [--datasets 45_intersections nine_intersections] [--envs 2048]
    python tools/ppo_eval_time.py --setup DATASET N_ENVS [--trace]                one setup, its lines (what the driver runs)

  (a) the same computation with reference-shaped torch modules, per agent: the stacks of the states and of the next states gathered from
      the store's obs with torch indexing, value_net on both, the actor on the states, Normal.log_prob.  It is chunked over time rows so
      that a chunk's stacks of one agent stay below --chunk-mb (the whole rollout's would be tens of GB on the wide dataset); the lines
      say how many chunks that made.  It uses nothing this repository did not have before the PPO evaluation kernel, so it runs unchanged
      on older commits: the baseline
  (b) PpoTargets.evaluate_store: one launch

The store is filled once by a captured episode of constant actions (what is evaluated does not matter for the time).  (a) and (b) run
ALTERNATELY in one process, --reps times each between two device events, behind a warm-up run of each.  The spread between the repetitions
of a case is the resolution of the comparison.  The driver runs every setup as a process of its own under its own `timeout`, chained with
`&&` (a step that fails or hangs ends the chain), and (b) once more per setup under `rocprofv3 --kernel-trace --stats` for the kernel's own
duration."""
import argparse
import glob
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK, MAX_DELTA = 5, 2.5


def torch_nets(torch, obs_w, act_w):
    nn = torch.nn

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc, self.ln = nn.Linear(STACK * obs_w, 64), nn.Linear(64, 64), nn.Linear(64, 64), nn.LayerNorm(64)
            self.fc_mu, self.fc_std = nn.Linear(64, act_w), nn.Linear(64, act_w)

        def forward(self, x):
            h = torch.relu(self.ln(self.fc(torch.relu(self.fc2(torch.relu(self.fc1(x.transpose(1, 2).flatten(1))))))))
            return self.fc_mu(h), nn.functional.softplus(self.fc_std(h)).clamp(1e-3, 10.0)

    class Value(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.fc, self.value_head = nn.Linear(STACK * obs_w, 64), nn.Linear(64, 64), nn.Linear(64, 64), nn.Linear(64, 1)

        def forward(self, x):
            return self.value_head(torch.relu(self.fc(torch.relu(self.fc2(torch.relu(self.fc1(x.transpose(1, 2).flatten(1))))))))

    make = lambda cls: cls().to("cuda").requires_grad_(False)
    return make(Actor), make(Value)


def ref_keys(sd):
    return {("encoder." + k if k[:3] in ("fc1", "fc2") else k): v for k, v in sd.items()}


def run_setup(dataset, n_envs, reps, chunk_mb, trace):
    import torch
    from torch.distributions import Normal

    sys.path.insert(0, ROOT)
    from pednstream_amd.rl_env import VecPedNetEnv

    env = VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3", seed=0, data_dir=os.path.join(ROOT, "data"), history="recent")
    agents = list(env.possible_agents)
    low, high = torch.as_tensor(env.action_low, device="cuda"), torch.as_tensor(env.action_high, device="cuda")
    const = (low + 0.5 * (high - low)).double().expand(n_envs, -1).contiguous()
    store = env.rollout_store()
    roll = env.capture(lambda obs: const, on_step=lambda obs, rew: store.record(const, None))
    env.reset(seed=3)
    store.begin()
    while not roll.step():
        pass
    T = store.finish()
    v = store.views()
    obs = v["obs"]
    torch.manual_seed(0)
    deltas = (torch.randn(T, n_envs, env.n_actions, device="cuda") * 0.7).clamp(-MAX_DELTA, MAX_DELTA)
    shapes = {aid: (env.obs_slices[aid].stop - env.obs_slices[aid].start, env.action_slices[aid].stop - env.action_slices[aid].start) for aid in agents}
    nets = {aid: torch_nets(torch, *shapes[aid]) for aid in agents}
    values_a, next_values_a = torch.zeros(T, n_envs, len(agents), device="cuda"), torch.zeros(T, n_envs, len(agents), device="cuda")
    logp_a = torch.zeros(T, n_envs, env.n_actions, device="cuda")
    widest = max(ow for ow, _ in shapes.values())
    chunk = max(1, min(T, int(chunk_mb * 2 ** 20 // (n_envs * STACK * widest * 4))))
    back = torch.arange(STACK, device="cuda") - (STACK - 1)

    def stacks(cols, t0, t1):
        """[(t1 - t0) * n_envs, STACK, obs_w]: the states of rows t0 .. t1 - 1 of one agent"""
        idx = (torch.arange(t0, t1, device="cuda")[:, None] + back[None, :]).clamp_(min=0)
        return obs[:, :, cols][idx].transpose(1, 2).reshape((t1 - t0) * n_envs, STACK, cols.stop - cols.start)

    def case_a():
        for i, aid in enumerate(agents):
            actor, value = nets[aid]
            o, a = env.obs_slices[aid], env.action_slices[aid]
            for t0 in range(0, T, chunk):
                t1 = min(T, t0 + chunk)
                states, next_states = stacks(o, t0, t1), stacks(o, t0 + 1, t1 + 1)
                next_values_a[t0:t1, :, i] = value(next_states).view(t1 - t0, n_envs)
                values_a[t0:t1, :, i] = value(states).view(t1 - t0, n_envs)
                mu, std = actor(states)
                logp_a[t0:t1, :, a] = Normal(mu, std).log_prob(deltas[t0:t1, :, a].reshape(-1, a.stop - a.start)).view(t1 - t0, n_envs, -1)

    cases = {"a": case_a}
    has_kernel = hasattr(env, "ppo_targets")                       # (older commits: the baseline alone)
    if has_kernel:
        actors = env.stacked_actors(kind="ppo", stack_size=STACK, delta_actions=True, max_delta=MAX_DELTA, seed=1)
        ppo = env.ppo_targets(actors)
        for aid in agents:
            actor, value = nets[aid]
            actors.load_state_dict(aid, ref_keys(actor.state_dict()))
            ppo.load_state_dict(aid, ref_keys(value.state_dict()))
        kept = {}

        def case_b():
            kept["logp"] = ppo.evaluate_store(store, actions=deltas)

        cases["b"] = case_b
    if trace:
        cases = {"b": cases["b"]}
    for fn in cases.values():                                      # warm-up (allocates)
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(reps):
        for name, fn in cases.items():                             # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    label = {"a": f"(a) torch modules, {len(agents)} agents, {-(-T // chunk)} chunks of {chunk} time rows", "b": "(b) evaluate_store"}
    head = f"{dataset} x {n_envs} envs, {T} rows, n_obs {env.n_obs}, obs_w {[ow for ow, _ in shapes.values()]}"
    for name, ts in times.items():
        print(f"{head} {label[name]}: {min(ts):9.3f} ms, best of {len(ts)}; all: " + " ".join(f"{t:.3f}" for t in ts) + f"; spread {max(ts) - min(ts):.3f}",
              flush=True)
    if has_kernel and not trace:                                   # the two compute the same thing (another summation order)
        vb = store.views()["values"]
        print(f"{head} mean |values (a) - (b)| {(values_a - vb[:T]).abs().mean().item():.3e}, |next_values (a) - values (b)[1:]| "
              f"{(next_values_a - vb[1:]).abs().mean().item():.3e} at mean |values| {vb.abs().mean().item():.3e}; mean |old_log_probs (a) - (b)| "
              f"{(logp_a - kept['logp']).abs().mean().item():.3e}", flush=True)
    env.close()


def kernel_stats(trace_dir):
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "ppo_" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs=2, metavar=("DATASET", "N_ENVS"))
    ap.add_argument("--trace", action="store_true", help="(b) alone: the run rocprofv3 wraps")
    ap.add_argument("--datasets", nargs="+", default=["45_intersections", "nine_intersections"])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk-mb", type=float, default=2048.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_eval_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "ppo_eval_trace"))
    args = ap.parse_args()
    if args.setup:
        run_setup(args.setup[0], int(args.setup[1]), args.reps, args.chunk_mb, args.trace)
        return 0
    out = shlex.quote(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/ppo_eval_time.py: the values of every state and the old log-probabilities of a filled rollout store for every agent, "
                f"eager, alternately ({args.reps} repetitions each behind a warm-up, device events)\n")
    rc = 0
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --reps {args.reps} --chunk-mb {args.chunk_mb}"
    for dataset in args.datasets:
        trace = os.path.join(args.trace_dir, dataset)
        steps = [f"timeout -k 10 240 {me} --setup {shlex.quote(dataset)} {args.envs} >> {out}",
                 f"timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d {shlex.quote(trace)} -- {me} --setup {shlex.quote(dataset)} {args.envs} --trace > /dev/null"]
        rc = subprocess.call(["bash", "-c", " && ".join(steps)])
        with open(args.out, "a") as f:
            if rc != 0:
                f.write(f"a step ended with status {rc}: the chain stopped there\n")
            else:
                f.write(f"kernel duration of (b) on {dataset}, rocprofv3 --kernel-trace --stats (ns):\n")
                f.write("\n".join(kernel_stats(trace)) + "\n")
        if rc != 0:
            break
    print(open(args.out).read())
    return rc


if __name__ == "__main__":
    sys.exit(main())
