#!/usr/bin/env python3
"""What do the reference's recurrent PPO agents cost on the device: one policy step of a captured rollout with the stateful LSTM actors,
and the gradient-free half of an update (the value LSTM over the states and over the next states, the actor LSTM and the old
log-probabilities) behind an episode?

    python tools/lstm_time.py [--out profiles/lstm_time.txt] [--datasets 45_intersections nine_intersections] [--envs 2048]
    python tools/lstm_time.py --setup DATASET N_ENVS --part act|update [--trace]     one measurement, its lines (what the driver runs)

  act     (a) reference-shaped torch modules per agent as the policy_fn of a captured rollout: an nn.LSTM step on the single frame with
              the state kept in two tensors, the heads, softplus and clamp, a normal draw, the delta clamp, the width and the clip
          (b) the same captured rollout with LstmActors.act: one launch
          microseconds per replayed policy step (env step included), --steps replays between two device events
  update  (a) reference-shaped torch modules per agent: nn.LSTM over the [n_envs, T, obs_w] batch of the states and of the next states
              (value network) and of the states (actor), the heads, Normal.log_prob
          (b) LstmPpoTargets.evaluate_store: one launch
          milliseconds per evaluation of a filled store

(a) uses nothing this repository did not have before the LSTM kernels.  (a) and (b) run ALTERNATELY in one process, --reps times each
between two device events, behind a warm-up of each.  The spread between the repetitions of a case is the resolution of the comparison.
The driver runs every measurement as a process of its own under its own `timeout`, chained with `&&` (a step that fails or hangs ends the
chain), and (b) once more per measurement under `rocprofv3 --kernel-trace --stats` for the kernels' own durations."""
import argparse
import glob
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DELTA = 2.5


def torch_nets(torch, obs_w, act_w):
    nn = torch.nn

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.lstm = nn.LSTM(input_size=obs_w, hidden_size=64, num_layers=1, batch_first=True)
            self.mean_head, self.std_head = nn.Linear(64, act_w), nn.Linear(64, act_w)

        def forward(self, x, hidden=None):
            out, hidden = self.lstm(x, hidden)
            f = torch.relu(out)
            return self.mean_head(f), nn.functional.softplus(self.std_head(f)).clamp(1e-3, 10.0), hidden

    class Value(nn.Module):
        def __init__(self):
            super().__init__()
            self.lstm, self.value_head = nn.LSTM(input_size=obs_w, hidden_size=64, num_layers=1, batch_first=True), nn.Linear(64, 1)

        def forward_all_steps(self, x):
            return self.value_head(torch.relu(self.lstm(x)[0]))

    make = lambda cls: cls().to("cuda").requires_grad_(False).eval()
    return make(Actor), make(Value)


def timed(torch, cases, reps, unit, scale, head, label):
    """Every case `reps` times, alternated, between device events; prints one line per case."""
    times = {name: [] for name in cases}
    for _ in range(reps):
        for name, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * scale)
    for name, ts in times.items():
        print(f"{head} {label[name]}: {min(ts):9.3f} {unit}, best of {len(ts)}; all: " + " ".join(f"{t:.3f}" for t in ts) + f"; spread {max(ts) - min(ts):.3f}",
              flush=True)


def make_env(dataset, n_envs):
    sys.path.insert(0, ROOT)
    from pednstream_amd.rl_env import VecPedNetEnv

    return VecPedNetEnv(dataset, n_envs=n_envs, obs_mode="option3", seed=0, data_dir=os.path.join(ROOT, "data"), history="recent")


def shapes_of(env):
    return {aid: (env.obs_slices[aid].stop - env.obs_slices[aid].start, env.action_slices[aid].stop - env.action_slices[aid].start) for aid in env.possible_agents}


def run_act(dataset, n_envs, reps, steps, trace):
    import torch

    cases, envs = {}, []
    torch.manual_seed(0)
    if not trace:
        env = make_env(dataset, n_envs)
        envs.append(env)
        shapes = shapes_of(env)
        nets = {aid: torch_nets(torch, *shapes[aid])[0] for aid in env.possible_agents}
        state = {aid: [torch.zeros(1, n_envs, 64, device="cuda") for _ in range(2)] for aid in env.possible_agents}
        low, high = torch.as_tensor(env.action_low, device="cuda"), torch.as_tensor(env.action_high, device="cuda")
        actions = torch.zeros(n_envs, env.n_actions, dtype=torch.float64, device="cuda")

        def policy(obs):
            for aid in env.possible_agents:
                o, a = env.obs_slices[aid], env.action_slices[aid]
                x = obs[:, o]
                mu, std, (h, c) = nets[aid](x.unsqueeze(1), (state[aid][0], state[aid][1]))
                state[aid][0].copy_(h)
                state[aid][1].copy_(c)
                raw = (mu[:, 0] + std[:, 0] * torch.randn_like(std[:, 0])).clamp(-MAX_DELTA, MAX_DELTA)
                width = x.reshape(n_envs, a.stop - a.start, -1)[:, :, -1]
                actions[:, a] = torch.minimum(torch.maximum(width + raw, low[a]), high[a]).double()
            return actions

        env.reset(seed=3)
        roll_a = env.capture(policy)
        cases["a"] = lambda: [roll_a.step() for _ in range(steps)]
    env_b = make_env(dataset, n_envs)
    envs.append(env_b)
    shapes = shapes_of(env_b)
    actors = env_b.lstm_actors(delta_actions=True, max_delta=MAX_DELTA, seed=1)
    for aid in env_b.possible_agents:
        actors.load_state_dict(aid, torch_nets(torch, *shapes[aid])[0].state_dict())
    env_b.reset(seed=3)
    actors.reset_hidden()
    roll_b = env_b.capture(lambda obs: actors.act(obs))
    cases["b"] = lambda: [roll_b.step() for _ in range(steps)]
    horizon = env_b.simulation_steps // env_b.action_gap
    warm = 10
    assert warm + reps * steps < horizon, f"{warm} + {reps} x {steps} policy steps do not fit an episode of {horizon}"
    for name, fn in cases.items():                                 # warm-up: the eager first step, the capture, a few replays
        roll = roll_b if name == "b" else roll_a
        for _ in range(warm):
            roll.step()
    torch.cuda.synchronize()
    label = {"a": f"(a) torch nn.LSTM step + heads + sampling, {len(shapes)} agents", "b": "(b) LstmActors.act"}
    head = f"{dataset} x {n_envs} envs, act, {steps} replayed policy steps, n_obs {env_b.n_obs}, obs_w {[ow for ow, _ in shapes.values()]}"
    timed(torch, cases, reps, "us per policy step", 1000.0 / steps, head, label)
    for env in envs:
        env.close()


def run_update(dataset, n_envs, reps, trace):
    import torch
    from torch.distributions import Normal

    env = make_env(dataset, n_envs)
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
    obs = store.views()["obs"]
    torch.manual_seed(0)
    deltas = (torch.randn(T, n_envs, env.n_actions, device="cuda") * 0.7).clamp(-MAX_DELTA, MAX_DELTA)
    shapes = shapes_of(env)
    nets = {aid: torch_nets(torch, *shapes[aid]) for aid in agents}
    values_a, next_values_a = torch.zeros(T, n_envs, len(agents), device="cuda"), torch.zeros(T, n_envs, len(agents), device="cuda")
    logp_a = torch.zeros(T, n_envs, env.n_actions, device="cuda")

    def case_a():
        for i, aid in enumerate(agents):
            actor, value = nets[aid]
            o, a = env.obs_slices[aid], env.action_slices[aid]
            x = obs[:, :, o].transpose(0, 1).contiguous()          # [n_envs, T + 1, obs_w]: an env is a batch row
            next_values_a[:, :, i] = value.forward_all_steps(x[:, 1:])[:, :, 0].t()
            values_a[:, :, i] = value.forward_all_steps(x[:, :T])[:, :, 0].t()
            mu, std, _ = actor(x[:, :T])
            logp_a[:, :, a] = Normal(mu, std).log_prob(deltas[:, :, a].transpose(0, 1)).transpose(0, 1)

    actors = env.lstm_actors(delta_actions=True, max_delta=MAX_DELTA, seed=1)
    ppo = env.lstm_ppo_targets(actors)
    for aid in agents:
        actors.load_state_dict(aid, nets[aid][0].state_dict())
        ppo.load_state_dict(aid, nets[aid][1].state_dict())
    kept = {}

    def case_b():
        kept.update(ppo.evaluate_store(store, actions=deltas))

    cases = {"b": case_b} if trace else {"a": case_a, "b": case_b}
    for fn in cases.values():                                      # warm-up (allocates)
        fn()
    torch.cuda.synchronize()
    label = {"a": f"(a) torch nn.LSTM over [n_envs, T, obs_w], {len(agents)} agents", "b": "(b) evaluate_store"}
    head = f"{dataset} x {n_envs} envs, update, {T} rows, n_obs {env.n_obs}, obs_w {[ow for ow, _ in shapes.values()]}"
    timed(torch, cases, reps, "ms", 1.0, head, label)
    if not trace:                                                  # the two compute the same thing (another summation order)
        print(f"{head} mean |values (a) - (b)| {(values_a - kept['values']).abs().mean().item():.3e}, |next_values (a) - (b)| "
              f"{(next_values_a - kept['next_values']).abs().mean().item():.3e} at mean |values| {kept['values'].abs().mean().item():.3e}; "
              f"mean |old_log_probs (a) - (b)| {(logp_a - kept['old_log_probs']).abs().mean().item():.3e}", flush=True)
    env.close()


def kernel_stats(trace_dir):
    out = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            lines = f.read().splitlines()
        out.append(lines[0])
        out += [l for l in lines[1:] if "lstm_" in l]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setup", nargs=2, metavar=("DATASET", "N_ENVS"))
    ap.add_argument("--part", choices=("act", "update"), default="update")
    ap.add_argument("--trace", action="store_true", help="(b) alone: the run rocprofv3 wraps")
    ap.add_argument("--datasets", nargs="+", default=["45_intersections", "nine_intersections"])
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=150, help="replayed policy steps per repetition of the act part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_time.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "outputs", "lstm_trace"))
    args = ap.parse_args()
    if args.setup:
        if args.part == "act":
            run_act(args.setup[0], int(args.setup[1]), args.reps, args.steps, args.trace)
        else:
            run_update(args.setup[0], int(args.setup[1]), args.reps, args.trace)
        return 0
    out = shlex.quote(args.out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("tools/lstm_time.py: a replayed policy step with the LSTM actors, and the values, next values and old log-probabilities of a "
                f"filled rollout store, torch modules against the LSTM launches, alternately ({args.reps} repetitions each behind a warm-up, "
                "device events)\n")
    rc = 0
    me = f"{shlex.quote(sys.executable)} {shlex.quote(os.path.abspath(__file__))} --reps {args.reps} --steps {args.steps}"
    for dataset in args.datasets:
        for part in ("act", "update"):
            trace = os.path.join(args.trace_dir, f"{dataset}_{part}")
            run = f"{me} --setup {shlex.quote(dataset)} {args.envs} --part {part}"
            steps = [f"timeout -k 10 240 {run} >> {out}",
                     f"timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d {shlex.quote(trace)} -- {run} --trace > /dev/null"]
            rc = subprocess.call(["bash", "-c", " && ".join(steps)])
            with open(args.out, "a") as f:
                if rc != 0:
                    f.write(f"a step ended with status {rc}: the chain stopped there\n")
                else:
                    f.write(f"kernel durations of (b), {part} on {dataset}, rocprofv3 --kernel-trace --stats (ns):\n")
                    f.write("\n".join(kernel_stats(trace)) + "\n")
            if rc != 0:
                break
        if rc != 0:
            break
    print(open(args.out).read())
    return rc


if __name__ == "__main__":
    sys.exit(main())
