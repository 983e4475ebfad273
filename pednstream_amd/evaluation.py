"""The reference's policy evaluation (rl/rl_utils.py:1513-1750: ``evaluate_agents`` / ``_evaluate_single_run``) for the rule-based
controllers, with every run an env of one ``VecPedNetEnv`` stepped on the device.

Run *i* is env *i*: its random numbers are those of replica ``replica_offset + i`` under the engine's RNG contract, and with
``randomize=True`` its scenario is env *i*'s draw of ``seed`` (``VecPedNetEnv.randomize``).  The controllers decide every action on the
device (``VecPedNetEnv.set_controllers``); the episode sums are float32 like the reference's ``episode_true_rewards[a] += rewards[a]``,
and the statistics over runs are computed from them with the reference's own numpy calls.
"""
import numpy as np

from .agents import RuleBasedGaterAgent, RuleBasedSeparatorAgent


def _vec_env(env):
    from .rl_env import VecPedNetEnv

    vec = getattr(env, "_vec", env)          # PedNetParallelEnv: its one-env VecPedNetEnv
    if not isinstance(vec, VecPedNetEnv):
        raise TypeError(f"evaluate_agents needs a VecPedNetEnv or PedNetParallelEnv, got {type(env).__name__}")
    return vec


def summarize_runs(agent_ids, episode_sums, verbose=False):
    """The reference's statistics over runs from per-run episode sums ``episode_sums[run][k]`` (float32) of ``agent_ids[k]``:
    the dict ``evaluate_agents`` returns (without metrics)."""
    all_runs, total_rewards, avg_rewards = [], [], []
    per_agent = {aid: [] for aid in agent_ids}
    for row in np.asarray(episode_sums, dtype=np.float32):
        ep = {aid: row[k] for k, aid in enumerate(agent_ids)}
        total = sum(ep.values())                      # rl_utils.py:1609-1610, Python's sum over np.float32
        avg = np.mean(list(ep.values()))
        all_runs.append({"episode_rewards": ep, "episode_normalized_rewards": dict(ep), "avg_reward": avg, "total_reward": total})
        total_rewards.append(total)
        avg_rewards.append(avg)
        for aid in agent_ids:
            per_agent[aid].append(ep[aid])
    n = len(all_runs)
    res = {
        "episode_rewards": {aid: np.mean(r) for aid, r in per_agent.items()},
        "episode_rewards_std": {aid: np.std(r) for aid, r in per_agent.items()} if n > 1 else {aid: 0.0 for aid in agent_ids},
        "avg_reward": np.mean(avg_rewards),
        "avg_reward_std": np.std(avg_rewards) if n > 1 else 0.0,
        "total_reward": np.mean(total_rewards),
        "total_reward_std": np.std(total_rewards) if n > 1 else 0.0,
        "all_runs": all_runs,
    }
    if verbose:
        print("=" * 60)
        print("Evaluation Results")
        if n > 1:
            print(f"  Number of runs: {n}")
        print("=" * 60)
        for aid in agent_ids:
            std = f" ± {res['episode_rewards_std'][aid]:.3f}" if n > 1 else ""
            print(f"  Agent {aid}: {res['episode_rewards'][aid]:.3f}{std}")
        pm = lambda k: f" ± {res[k + '_std']:.3f}" if n > 1 else ""
        print(f"  Average reward: {res['avg_reward']:.3f}{pm('avg_reward')}")
        print(f"  Total reward: {res['total_reward']:.3f}{pm('total_reward')}")
        print("=" * 60)
    return res


def evaluate_agents(env, agents, delta_actions=False, deterministic=True, seed=None, no_control=False, randomize=False,
                    save_dir=None, verbose=True, num_runs=None, metrics=False):
    """``rl_utils.evaluate_agents`` with the reference's signature and result dict, every run an env of ``env`` (``num_runs``:
    the first that many envs; default all of them).  ``agents``: ``{agent_id: RuleBasedGaterAgent | RuleBasedSeparatorAgent}``;
    ``no_control=True`` runs the same episodes without any action.  ``metrics=True`` (needs ``track_metrics=True``) adds each
    run's evaluation metrics (``pednstream_amd.metrics.network_metrics`` of its env) as ``all_runs[i]["metrics"]``.

    Refused: ``delta_actions`` (only absolute actions of the rule-based agents), ``save_dir`` (no per-run output files), and any other
    kind of agent -- a torch policy runs on the device through ``VecPedNetEnv.capture``.  ``deterministic`` does not change a
    rule-based agent."""
    if delta_actions:
        raise ValueError("evaluate_agents: delta_actions is not supported (the rule-based agents act with absolute widths)")
    if save_dir is not None:
        raise ValueError("evaluate_agents: save_dir is not supported; save a run with PedNetParallelEnv.save")
    for aid, agent in agents.items():
        if agent is not None and not isinstance(agent, (RuleBasedGaterAgent, RuleBasedSeparatorAgent)):
            raise TypeError(f"evaluate_agents runs RuleBasedGaterAgent / RuleBasedSeparatorAgent on the device; {aid} is a "
                            f"{type(agent).__name__} (a torch policy goes through VecPedNetEnv.capture)")
    vec = _vec_env(env)
    n_runs = vec.n_envs if num_runs is None else int(num_runs)
    if not 1 <= n_runs <= vec.n_envs:
        raise ValueError(f"num_runs must be in 1..n_envs = {vec.n_envs}, got {num_runs}")
    if metrics and not vec.track_metrics:
        raise ValueError("metrics=True needs an env constructed with track_metrics=True")
    for aid in agents:
        if aid not in vec.action_slices:
            raise ValueError(f"Unknown agent: {aid}")
    if verbose and n_runs > 1:
        print(f"Running {n_runs} evaluation runs...")
    vec.set_controllers({} if no_control else agents)
    vec.reset(options={"randomize": True} if randomize else None, seed=seed)
    vec.step_controlled(fetch=False)
    sums = vec.episode_rewards()[:n_runs]
    ids = list(agents.keys())
    cols = [vec.possible_agents.index(aid) for aid in ids]
    res = summarize_runs(ids, sums[:, cols], verbose=verbose)
    if metrics:
        from .metrics import replica

        m = vec.episode_metrics()
        for i, run in enumerate(res["all_runs"]):
            run["metrics"] = replica(m, i)
    return res
