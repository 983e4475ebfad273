"""The running-normalisation contract restated in numpy -- what pednstream_amd/csrc/pedn_norm.hpp must compute bit
for bit, the way oracle/rand_contract.py restates the randomiser.  Only IEEE binary64 + - * / sqrt on scalars and arrays; nothing here
calls np.sum / np.mean / np.var, whose order is numpy's own business.

    model = NormModel(n_envs, tracked, agent_of_column, n_agents, norm_obs=True, norm_reward=False, ...)
    model.reset()                                   # zeroes the discounted returns, keeps the statistics
    obs_n = model.observe(obs)                      # [n_envs, n_obs] float32 -> float32
    rew_n = model.rewards(rew, terminated)          # [n_envs, n_agents] float32 -> float32
"""
import numpy as np

STRANDS = 64


def _tree(nodes):
    """Neighbours are paired level by level; a node without a right neighbour moves up as it is."""
    while len(nodes) > 1:
        nxt = [nodes[i] + nodes[i + 1] for i in range(0, len(nodes) - 1, 2)]
        if len(nodes) % 2:
            nxt.append(nodes[-1])
        nodes = nxt
    return nodes[0]


def fixed_sum(x):
    """S: x [N, ...] float64 summed over axis 0 in the contract's order -- strand s adds rows s, s + 64, ... in increasing order starting
    from its first row; the min(N, 64) strand sums are the leaves of a tree that pairs neighbours."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    leaves = []
    for s in range(min(n, STRANDS)):
        acc = x[s].copy()
        for e in range(s + STRANDS, n, STRANDS):
            acc = acc + x[e]
        leaves.append(acc)
    return _tree(leaves)


def batch_moments(x):
    """(mean, variance) over axis 0 of x [N, ...] (values already float64)."""
    x = np.asarray(x, dtype=np.float64)
    n = float(x.shape[0])
    bm = fixed_sum(x) / n
    d = x - bm
    return bm, fixed_sum(d * d) / n


def merge(mean, var, count, bm, bv, n):
    """RunningMeanStd._update_from_moments (rl/rl_utils.py:74-83), operation for operation."""
    n = float(n)
    delta = bm - mean
    tot = count + n
    mean = mean + delta * n / tot
    m2 = var * count + bv * n + delta * delta * count * n / tot
    return mean, m2 / tot, tot


class NormModel:
    def __init__(self, n_envs, tracked, agent_of_column, n_agents, norm_obs=True, norm_reward=False, clip_obs=50.0, clip_reward=10.0,
                 gamma=0.99, training=True):
        self.n_envs, self.n_agents = int(n_envs), int(n_agents)
        self.tracked = np.asarray(tracked, dtype=bool)
        self.agent_of_column = np.asarray(agent_of_column, dtype=np.int64)
        self.norm_obs, self.norm_reward, self.training = bool(norm_obs), bool(norm_reward), bool(training)
        self.clip_obs, self.clip_reward, self.gamma = float(clip_obs), float(clip_reward), float(gamma)
        n_obs = len(self.tracked)
        self.mean, self.var, self.count = np.zeros(n_obs), np.ones(n_obs), np.full(n_obs, 1e-4)     # (one count per column: equal within an agent)
        self.ret = np.zeros((self.n_envs, self.n_agents))
        self.ret_mean, self.ret_var, self.ret_count = 0.0, 1.0, 1e-4

    def reset(self):
        self.ret[:] = 0.0

    def observe(self, obs):
        obs = np.asarray(obs, dtype=np.float32)
        assert obs.shape == (self.n_envs, len(self.tracked))
        if not self.norm_obs:
            return obs.copy()
        tr = self.tracked
        x = obs[:, tr].astype(np.float64)
        if self.training:
            bm, bv = batch_moments(x)
            self.mean[tr], self.var[tr], self.count[tr] = merge(self.mean[tr], self.var[tr], self.count[tr], bm, bv, self.n_envs)
        out = obs.copy()
        with np.errstate(invalid="ignore"):
            out[:, tr] = np.clip((x - self.mean[tr]) / np.sqrt(self.var[tr] + 1e-8), -self.clip_obs, self.clip_obs).astype(np.float32)
        return out

    def rewards(self, rew, terminated):
        rew = np.asarray(rew, dtype=np.float32)
        assert rew.shape == (self.n_envs, self.n_agents)
        if not self.norm_reward:
            return rew.copy()
        out = np.empty_like(rew)
        keep = 1.0 - float(bool(terminated))
        for a in range(self.n_agents):            # agent a + 1 sees the statistics agent a left
            r = rew[:, a].astype(np.float64)
            self.ret[:, a] = r + self.gamma * self.ret[:, a] * keep
            if self.training:
                bm, bv = batch_moments(self.ret[:, a])
                self.ret_mean, self.ret_var, self.ret_count = merge(self.ret_mean, self.ret_var, self.ret_count, bm, bv, self.n_envs)
            out[:, a] = np.clip(r / np.sqrt(self.ret_var + 1e-8), -self.clip_reward, self.clip_reward).astype(np.float32)
        return out

    def stats(self, agent_ids):
        """The reference's dict layout (rl_utils.py:273-287): per agent mean / var / count over its tracked columns."""
        out = {"obs_rms": {}}
        for a, aid in enumerate(agent_ids):
            cols = np.flatnonzero((self.agent_of_column == a) & self.tracked)
            out["obs_rms"][aid] = {"mean": self.mean[cols].tolist(), "var": self.var[cols].tolist(),
                                   "count": float(self.count[cols[0]]) if len(cols) else 1e-4}
        if self.norm_reward:
            out["ret_rms"] = {"mean": float(self.ret_mean), "var": float(self.ret_var), "count": float(self.ret_count)}
        return out
