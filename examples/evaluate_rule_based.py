"""The reference's baseline comparison (rl/evaluate_and_visualize.py: run_tests) on the device: the rule-based gater agents
(threshold 3, option2) against no control on nine_intersections, every run one env of a 1024-env batch, with the evaluation metrics of
every run -- no observation or action crosses to the host during the episodes.

    python examples/evaluate_rule_based.py [n_envs]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pednstream_amd.agents import RuleBasedGaterAgent  # noqa: E402
from pednstream_amd.evaluation import evaluate_agents  # noqa: E402
from pednstream_amd.rl_env import VecPedNetEnv  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    np.random.seed(0)
    env = VecPedNetEnv("nine_intersections", n_envs=B, obs_mode="option2", track_metrics=True, data_dir=os.path.join(ROOT, "data"))
    am = env.agent_manager
    agents = {aid: RuleBasedGaterAgent(am.get_gater_outgoing_links(aid), env.obs_mode, threshold_density=3) for aid in am.gater_agents}
    for label, no_control in (("rule_based", False), ("no_control", True)):
        t0 = time.perf_counter()
        res = evaluate_agents(env, agents, no_control=no_control, verbose=False, metrics=True)
        dt = time.perf_counter() - t0
        served = np.array([run["metrics"]["served_trips_rate"]["served_trips_rate"] for run in res["all_runs"]])
        delay = np.array([run["metrics"]["total_network_delay"]["total_delay"] for run in res["all_runs"]])
        print(f"{label:11s} {B} runs in {dt:.2f} s: total reward {res['total_reward']:.4g} ± {res['total_reward_std']:.3g}, "
              f"served-trip rate {served.mean():.4f}, total delay {delay.mean():.4g}")
    env.close()


if __name__ == "__main__":
    main()
