"""Record what the reference's RunningNormalizeWrapper (rl/rl_utils.py:86-300) returns for a few golden RL episodes:
tests/golden/norm_<case>_<flags>.npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  The REAL classes are loaded through oracle/ref_harness.load_reference_rl() (a bare `rl`
package, rl.rl_utils imported under it) and wrapped around a stub env that replays an existing RL golden: the reference's own
AgentManager / ObservationBuilder for the scenario (agent types, features_per_link, the reset observation), then row after row of
state_rl_obs / state_rl_rewards / state_rl_terminated.  The stub hands out what pednstream_amd.PedNetParallelEnv hands out: float32
observation arrays, Python-float rewards for every agent, bool terminations.  `training` is switched off for the last quarter of the steps.
Only recorded results are stored:

    reset_obs [O] f32 (raw), reset_obs_n [O] f32, obs_n [K, O] f32, rew_n [K, A] f64 (as the reference returns them; the contract's
    output is their float32 rounding), true_rew [K, A] f64, mean / var [tracked columns, agent after agent] f64, count [A] f64,
    ret_rms [3] f64 (norm_reward only), info_json

    python tools/gen_norm_goldens.py [case ...]
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("rl_nine_opt3", "rl_corridor_opt1", "rl_i45_episode")
FLAGS = {"obs": dict(norm_obs=True, norm_reward=False), "obsrew": dict(norm_obs=True, norm_reward=True)}


class _Space:
    def __init__(self, n):
        self.shape = (n,)


class ReplayEnv:
    """The attributes RunningNormalizeWrapper reads off its env, served from a golden."""

    def __init__(self, z, info):
        ref = rh.load_reference()
        rl = info["rl"]
        np.random.seed(info["np_seed"])
        cwd = os.getcwd()
        os.chdir(rh.REF_ROOT)       # NetworkEnvGenerator() reads data/ relative to the working directory
        try:
            net = ref["env"].NetworkEnvGenerator().create_network(info["scenario"])
        finally:
            os.chdir(cwd)
        shim = rh.RefEnvShim(net, obs_mode=rl["obs_mode"], normalize_obs=rl["normalize"], action_gap=rl["action_gap"])
        self.agent_manager, self.obs_builder, self.possible_agents = shim.agent_manager, shim.obs_builder, list(shim.possible_agents)
        assert self.possible_agents == [a["id"] for a in rl["agents"]]
        self._reset_obs = {a: np.asarray(shim.obs_builder.build_observation(a, 1), dtype=np.float32) for a in self.possible_agents}
        self._slices, o = {}, 0
        for a in self.possible_agents:
            self._slices[a] = slice(o, o + len(self._reset_obs[a]))
            o += len(self._reset_obs[a])
        self._obs, self._rew, self._term = z["state_rl_obs"], z["state_rl_rewards"], z["state_rl_terminated"]
        assert self._obs.shape[1] == o
        self._k = 0

    def observation_space(self, aid):
        return _Space(self._slices[aid].stop - self._slices[aid].start)

    def reset(self, **kw):
        self._k = 0
        return {a: o.copy() for a, o in self._reset_obs.items()}, {a: {} for a in self.possible_agents}

    def step(self, actions):
        k = self._k
        self._k += 1
        obs = {a: self._obs[k, sl].copy() for a, sl in self._slices.items()}
        rew = {a: float(self._rew[k, i]) for i, a in enumerate(self.possible_agents)}
        term = {a: bool(self._term[k]) for a in self.possible_agents}
        return obs, rew, term, {a: False for a in self.possible_agents}, {a: {} for a in self.possible_agents}


def record(case, flags):
    z = np.load(os.path.join(GOLDEN, case + ".npz"))
    info = json.loads(str(z["info_json"]))
    rh.load_reference_rl()
    utils = importlib.import_module("rl.rl_utils")
    env = ReplayEnv(z, info)
    wrapped = utils.RunningNormalizeWrapper(env, clip_obs=50.0, clip_reward=10.0, gamma=0.99, training=True, **FLAGS[flags])
    agents = env.possible_agents
    flat = lambda d: np.concatenate([np.asarray(d[a]) for a in agents])
    steps = len(z["state_rl_obs"])
    frozen_from = steps - steps // 4
    obs0, _ = wrapped.reset()
    obs_n, rew_n, true_rew = [], [], []
    for k in range(steps):
        if k == frozen_from:
            wrapped.set_training(False)
        obs, rew, term, trunc, infos = wrapped.step({})
        assert flat(obs).dtype == np.float32
        obs_n.append(flat(obs))
        rew_n.append([float(np.asarray(rew[a]).reshape(-1)[0]) for a in agents])      # (shape (1,) once ret_rms has been updated)
        true_rew.append([float(infos[a]["true_reward"]) for a in agents])
    stats = wrapped.get_normalization_stats()
    out = {"reset_obs": flat(env._reset_obs), "reset_obs_n": flat(obs0), "obs_n": np.array(obs_n, dtype=np.float32),
           "rew_n": np.array(rew_n, dtype=np.float64), "true_rew": np.array(true_rew, dtype=np.float64),
           "mean": np.concatenate([np.asarray(stats["obs_rms"][a]["mean"], dtype=np.float64) for a in agents]),
           "var": np.concatenate([np.asarray(stats["obs_rms"][a]["var"], dtype=np.float64) for a in agents]),
           "count": np.array([stats["obs_rms"][a]["count"] for a in agents], dtype=np.float64)}
    if "ret_rms" in stats:
        out["ret_rms"] = np.array([stats["ret_rms"][k] for k in ("mean", "var", "count")], dtype=np.float64)
    out["info_json"] = np.array(json.dumps({"case": case, "flags": FLAGS[flags], "clip_obs": 50.0, "clip_reward": 10.0, "gamma": 0.99,
                                            "steps": steps, "frozen_from": frozen_from, "agents": agents, "numpy": np.__version__}))
    path = os.path.join(GOLDEN, f"norm_{case[3:]}_{flags}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    for c in sys.argv[1:] or CASES:
        for f in FLAGS:
            record(c, f)
