"""The reference's running normalisation (rl/rl_utils.py:57-300) with the statistics kept -- and updated -- on the device.

  RunningMeanStd            host-side mean / var / count with the reference's update: for loading, saving and inspecting statistics
  RunningNormalizeWrapper   the reference's wrapper around ``PedNetParallelEnv`` (same signature, same dict API, ``__getattr__`` delegates
                            to the env, ``infos[aid]['true_reward']``).  It does not normalise on the host: it switches on
                            ``VecPedNetEnv.set_running_norm`` of the env underneath, whose observation launch is followed by the
                            normalisation kernel (pednstream_amd/csrc/pedn_norm.hpp).  With its one env this reproduces the reference's
                            wrapper bit for bit (tests/golden/norm_*.npz); a batch user calls ``set_running_norm`` on the batched env.
"""
import numpy as np


class RunningMeanStd:
    """rl/rl_utils.py:57-83."""

    def __init__(self, epsilon=1e-4, shape=()):
        self.mean = np.zeros(shape, dtype=np.float64)
        self.var = np.ones(shape, dtype=np.float64)
        self.count = epsilon

    def update(self, x):
        x = np.asarray(x)
        self._update_from_moments(np.mean(x, axis=0), np.var(x, axis=0), x.shape[0])

    def _update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        total_count = self.count + batch_count
        self.mean = self.mean + delta * batch_count / total_count
        m2 = self.var * self.count + batch_var * batch_count + np.square(delta) * self.count * batch_count / total_count
        self.var = m2 / total_count
        self.count = total_count


class RunningNormalizeWrapper:
    def __init__(self, env, norm_obs=True, norm_reward=False, clip_obs=50.0, clip_reward=10.0, gamma=0.99, training=True):
        vec = getattr(env, "_vec", None)
        if vec is None or not hasattr(vec, "set_running_norm"):
            raise TypeError("RunningNormalizeWrapper wraps a pednstream_amd PedNetParallelEnv (a batched env calls set_running_norm itself)")
        self.env = env
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward, self.gamma, self.training = clip_obs, clip_reward, gamma, bool(training)
        vec.set_running_norm(norm_obs=self.norm_obs, norm_reward=self.norm_reward, clip_obs=clip_obs, clip_reward=clip_reward,
                             gamma=gamma, training=training)

    def __getattr__(self, name):
        """Delegate attribute access to the wrapped environment (rl_utils.py:148-150)."""
        return getattr(self.env, name)

    @property
    def _on(self):
        return self.norm_obs or self.norm_reward

    def reset(self, **kwargs):
        return self.env.reset(**kwargs)          # (the env underneath hands out the normalised reset observation)

    def step(self, actions):
        obs, rewards, terms, truncs, infos = self.env.step(actions)
        true = self.env._vec.true_rewards()[0] if self._on else None
        for i, aid in enumerate(self.env.possible_agents):
            infos.setdefault(aid, {})["true_reward"] = float(true[i]) if self._on else rewards[aid]
        return obs, rewards, terms, truncs, infos

    def set_training(self, training):
        self.training = bool(training)
        if self._on:
            self.env._vec.set_training(training)

    def get_normalization_stats(self):
        if self._on:
            return self.env._vec.get_normalization_stats()
        return {"obs_rms": {aid: {"mean": r.mean.tolist(), "var": r.var.tolist(), "count": r.count} for aid, r in self.obs_rms.items()}}

    def set_normalization_stats(self, stats):
        if self._on:
            self.env._vec.set_normalization_stats(stats)

    @property
    def obs_rms(self):
        """{agent: RunningMeanStd}: host snapshots of the device statistics (tracked features only, like the reference's shapes)."""
        vec = self.env._vec
        out = {}
        if self._on:
            stats = vec.get_normalization_stats()["obs_rms"]
        else:
            tracked, agent = vec.norm_layout()
            stats = {aid: None for aid in vec.possible_agents}
        for i, aid in enumerate(vec.possible_agents):
            d = stats[aid]
            rms = RunningMeanStd(shape=(len(d["mean"]) if d else int((tracked & (agent == i)).sum()),))
            if d:
                rms.mean, rms.var, rms.count = np.array(d["mean"]), np.array(d["var"]), d["count"]
            out[aid] = rms
        return out

    @property
    def ret_rms(self):
        if not self.norm_reward:
            return None
        d = self.env._vec.get_normalization_stats()["ret_rms"]
        rms = RunningMeanStd(shape=())
        rms.mean, rms.var, rms.count = np.float64(d["mean"]), np.float64(d["var"]), d["count"]
        return rms
