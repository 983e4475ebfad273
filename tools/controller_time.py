"""Time of an env step whose actions the rule-based controllers decide on the device (VecPedNetEnv.step_controlled), against the plain
device-action step with a constant action tensor (step_device(sync=False)) and against the host loop the reference runs (fetch the
observations, numpy take_action per env and agent, upload the actions: step).

    python tools/controller_time.py [n_envs] [steps] [out]      (default 2048 envs, 200 env steps; profiles/controller_time.txt)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pednstream_amd.agents import RuleBasedGaterAgent, RuleBasedSeparatorAgent  # noqa: E402
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402


def agents_of(env):
    am = env.agent_manager
    out = {}
    for aid in env.possible_agents:
        if am.get_agent_type(aid) == "gate":
            out[aid] = RuleBasedGaterAgent(am.get_gater_outgoing_links(aid), "option2", threshold_density=3)
        else:
            out[aid] = RuleBasedSeparatorAgent(am.get_separator_links(aid)[0].width, use_smoothing=True, buffer_size=5)
    return out


def main():
    import torch

    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    lines = [f"rule-based controllers on the device: us per env step, {B} envs, {K} env steps after a warm-up of 20 (median of 3)"]
    for name in ("45_intersections", "nine_intersections", "one_intersection_v0"):
        np.random.seed(0)
        env = VecPedNetEnv(name, n_envs=B, obs_mode="option2", data_dir=os.path.join(ROOT, "data"))
        env.set_controllers(agents_of(env))
        eng = env.network.engine()
        ctrl, dev = [], []
        for _ in range(3):
            env.reset()
            env.step_controlled(20, fetch=False)
            eng.synchronize()
            t0 = time.perf_counter()
            env.step_controlled(K, fetch=False)
            eng.synchronize()
            ctrl.append((time.perf_counter() - t0) / K * 1e6)
        a = torch.full((B, env.n_actions), 2.0, dtype=torch.float64, device="cuda")
        for _ in range(3):
            env.reset()
            for _ in range(20):
                env.step_device(a, sync=False)
            torch.cuda.synchronize()
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                env.step_device(a, sync=False)
            torch.cuda.synchronize()
            eng.synchronize()
            dev.append((time.perf_counter() - t0) / K * 1e6)
        # the reference's loop: every env's agents on the host (a few steps: it is slow)
        per_env = [agents_of(env) for _ in range(B)]
        obs, _ = env.reset()
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            row = np.full((B, env.n_actions), np.nan)
            for r in range(B):
                for aid, ag in per_env[r].items():
                    row[r, env.action_slices[aid]] = ag.take_action(obs[r, env.obs_slices[aid]])
            obs, *_ = env.step(row)
            host.append((time.perf_counter() - t0) * 1e6)
        c, d, h = np.median(ctrl), np.median(dev), np.median(host)
        lines.append(f"{name:22s} agents {len(env.possible_agents):3d}  step_controlled {c:8.1f}   step_device(constant) {d:8.1f}   "
                     f"ratio {c / d:5.2f}   host loop {h:12.0f}")
        env.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 3:                     # an output file, e.g. profiles/controller_time.txt
        with open(sys.argv[3], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
