"""The arithmetic contract of PPO's rollout evaluation (pednstream_amd/csrc/pedn_ppo.hpp) restated in numpy: TEST
INFRASTRUCTURE.  The actor and the layers are those of tests/actor_model.py (section 14); every float32 product and sum is one rounded
operation; the log-probability is evaluated in float64 from the float32 values and rounded once.

    stacks(obs, S)                       -> [T + 1, N, S, n_obs]: the state of every row, frames max(t - (S - 1) + s, 0), oldest first
    value(sd, x)                         -> v float32 [B]                  x: [B, S, obs_w]
    log_prob(a, mu, std)                 -> float32, torch's Normal(mu, std).log_prob(a)
    evaluate(agents, actor_sds, value_sds, obs, actions, S, min_std, max_std) -> dict of values, mu, std, old_log_probs
"""
import math

import numpy as np

import actor_model as am

F = np.float32
LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
VALUE_KEYS = ("encoder.fc1", "encoder.fc2", "fc", "value_head")


def stack_times(T, S):
    """int [T + 1, S]: the time rows of the frames of the state of row t."""
    return np.maximum(np.arange(T + 1)[:, None] - (S - 1) + np.arange(S)[None, :], 0)


def stacks(obs, S):
    """[T + 1, N, n_obs] -> [T + 1, N, S, n_obs]: the reference's deque, S copies of the reset observation, then one append per step."""
    obs = np.asarray(obs, dtype=F)
    return np.ascontiguousarray(np.swapaxes(obs[stack_times(obs.shape[0] - 1, S)], 1, 2))


def value(sd, x):
    """v [B] of the value network whose state dict (reference keys, arrays) is sd: value_head(relu(fc(encoder(x)))), no LayerNorm."""
    p = lambda k: (sd[k + ".weight"], sd[k + ".bias"])
    zs = am.relu(am.linear(*p("encoder.fc1"), am.flatten_stack(x)))
    zs = am.relu(am.linear(*p("encoder.fc2"), zs))
    h = am.linear(*p("fc"), zs)
    return am.linear(*p("value_head"), am.relu(h))[:, 0]


def log_prob(a, mu, std):
    """-((a - mu)^2) / (2 std^2) - log(std) - log(sqrt(2 pi)) in float64 from the float32 values, rounded once."""
    A, M, S = (np.asarray(v, dtype=F).astype(np.float64) for v in (a, mu, std))
    with np.errstate(all="ignore"):
        return (-((A - M) * (A - M)) / (2.0 * (S * S)) - np.log(S) - LOG_SQRT_2PI).astype(F)


def evaluate(agents, actor_sds, value_sds, obs, actions, S, min_std=1e-3, max_std=10.0):
    """values [T + 1, N, n_agents], mu, std, old_log_probs [T, N, n_actions] float32 of obs [T + 1, N, n_obs] and actions [T, N,
    n_actions] (float32, or float64 read as float32); agents = [(obs0, obs_w, act0, act_w)].  Columns no agent owns stay zero."""
    obs = np.asarray(obs, dtype=F)
    act = np.asarray(actions).astype(F)
    T, N = obs.shape[0] - 1, obs.shape[1]
    st = stacks(obs, S).reshape((T + 1) * N, S, obs.shape[2])
    out = {"values": np.zeros((T + 1, N, len(agents)), dtype=F)}
    for k in ("mu", "std", "old_log_probs"):
        out[k] = np.zeros(act.shape, dtype=F)
    for i, ((o0, ow, a0, aw), asd, vsd) in enumerate(zip(agents, actor_sds, value_sds)):
        x = st[:, :, o0:o0 + ow]
        out["values"][:, :, i] = value(vsd, x).reshape(T + 1, N)
        mu, _, std = am.forward("ppo", asd, x[:T * N], min_std, max_std)
        sl = slice(a0, a0 + aw)
        out["mu"][:, :, sl], out["std"][:, :, sl] = mu.reshape(T, N, aw), std.reshape(T, N, aw)
        out["old_log_probs"][:, :, sl] = log_prob(act[:, :, sl], out["mu"][:, :, sl], out["std"][:, :, sl])
    return out
