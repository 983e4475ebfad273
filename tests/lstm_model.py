"""The arithmetic contract of the LSTM PPO agents (pednstream_amd/csrc/pedn_lstm.hpp) restated in numpy: TEST
INFRASTRUCTURE.  One nn.LSTM layer of 64 units, gate rows i, f, g, o.  Every float32 product and sum is one rounded operation; a gate row
sums bias_ih + bias_hh, then W_ih x, then W_hh h, k ascending, into one accumulator; sigmoid and tanh are evaluated in float64 from the
float32 value with the oracle's exp (pedn_oracle_exp, what the device's pedn_exp restates) and rounded once.  The heads, the tail, the
log-probability and the Philox draw are tests/actor_model.py's and tests/ppo_eval_model.py's (sections 14 and 16).

    step(sd, x, h, c)                         -> h', c'                                   x: [B, obs_w], h / c: [B, 64] float32
    actor_heads(sd, h, min_std, max_std)      -> mu, z (the pre-softplus value), std      [B, act_w]
    value_head(sd, h)                         -> v [B]
    run(sd, xs, with_c=False)                 -> hs [T, B, 64] (and cs) from a zero state  xs: [T, B, obs_w]
    noise(seed, g, c, d)                      -> eps float32 (site byte 0x74)
    evaluate(agents, actor_sds, value_sds, obs, actions, ...) -> values, next_values, mu, std, old_log_probs
    gae_next(rewards, values, next_values, dones, gamma, lmbda) -> td_target, adv
"""
import numpy as np

import actor_model as am
import oracle_driver as od
import ppo_eval_model as pm
import rollout_model as rm

F = np.float32
H = 64
NOISE_SITE = 0x74
_exp = None


def exp(x):
    """The oracle's exp on a float64 array."""
    global _exp
    if _exp is None:
        _exp = np.frompyfunc(od.lib().pedn_oracle_exp, 1, 1)
    x = np.asarray(x, dtype=np.float64)
    return _exp(x).astype(np.float64).reshape(x.shape)


def sigmoid64(z):
    """1 / (1 + exp(-z)) in float64 (z float32)."""
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + exp(-np.asarray(z, dtype=F).astype(np.float64)))


def tanh64(z):
    """copysign(t, z), t = a - a a a / 3 below 2^-13, else (1 - e) / (1 + e) with e = exp(-2 a), a = |z|, in float64 (z float32)."""
    z = np.asarray(z, dtype=F).astype(np.float64)
    a = np.abs(z)
    with np.errstate(all="ignore"):
        e = exp(-2.0 * a)
        t = np.where(a < 2.0 ** -13, a - a * a * a / 3.0, (1.0 - e) / (1.0 + e))
    return np.copysign(t, z)


def sigmoid(z):
    return sigmoid64(z).astype(F)


def tanh(z):
    return tanh64(z).astype(F)


def gates(sd, x, h):
    """[B, 256] float32: the pre-activations of the gate rows."""
    wih, whh = np.asarray(sd["lstm.weight_ih_l0"], dtype=F), np.asarray(sd["lstm.weight_hh_l0"], dtype=F)
    x, h = np.asarray(x, dtype=F), np.asarray(h, dtype=F)
    with np.errstate(all="ignore"):
        bias = np.asarray(sd["lstm.bias_ih_l0"], dtype=F) + np.asarray(sd["lstm.bias_hh_l0"], dtype=F)
        acc = np.broadcast_to(bias, (x.shape[0], 4 * H)).astype(F)
        for k in range(wih.shape[1]):
            acc = acc + wih[None, :, k] * x[:, k, None]
        for k in range(H):
            acc = acc + whh[None, :, k] * h[:, k, None]
    assert acc.dtype == F
    return acc


def step(sd, x, h, c):
    """One step of the layer: h', c' [B, 64] float32."""
    a = gates(sd, x, h)
    i, f, g, o = sigmoid(a[:, :H]), sigmoid(a[:, H:2 * H]), tanh(a[:, 2 * H:3 * H]), sigmoid(a[:, 3 * H:])
    with np.errstate(all="ignore"):
        c2 = (f * np.asarray(c, dtype=F)) + (i * g)
        h2 = o * tanh(c2)
    assert c2.dtype == F and h2.dtype == F
    return h2, c2


def run(sd, xs, with_c=False):
    """hs [T, B, 64] (with_c: and cs) of the layer over xs [T, B, obs_w] from h = c = +0.0."""
    xs = np.asarray(xs, dtype=F)
    h = c = np.zeros((xs.shape[1], H), dtype=F)
    hs, cs = (np.empty((xs.shape[0], xs.shape[1], H), dtype=F) for _ in range(2))
    for t in range(xs.shape[0]):
        h, c = step(sd, xs[t], h, c)
        hs[t], cs[t] = h, c
    return (hs, cs) if with_c else hs


def actor_heads(sd, h, min_std=1e-3, max_std=10.0):
    """mu, z, std [B, act_w] float32 on relu(h)."""
    r = am.relu(h)
    mu = am.linear(sd["mean_head.weight"], sd["mean_head.bias"], r)
    z = am.linear(sd["std_head.weight"], sd["std_head.bias"], r)
    return mu, z, am.clip(am.softplus(z), F(min_std), F(max_std))


def value_head(sd, h):
    return am.linear(sd["value_head.weight"], sd["value_head.bias"], am.relu(h))[:, 0]


def noise(seed, g, c, d):
    """eps of global env g, action column c, draw d: actor_model.noise with this path's site byte."""
    keep = am.NOISE_SITE
    am.NOISE_SITE = NOISE_SITE
    try:
        return am.noise(seed, g, c, d)
    finally:
        am.NOISE_SITE = keep


def widths(x, act_w):
    """[B, obs_w] -> [B, act_w]: obs.reshape(act_dim, -1)[:, -1]."""
    x = np.asarray(x, dtype=F)
    return x.reshape(x.shape[0], act_w, -1)[:, :, -1]


def evaluate(agents, actor_sds, value_sds, obs, actions, min_std=1e-3, max_std=10.0):
    """values, next_values [T, N, n_agents], mu, z (the pre-softplus value), std, old_log_probs [T, N, n_actions] and h, c [n_agents, T,
    N, 64] (the actor's state behind every step) of obs [T + 1, N, n_obs] and actions [T, N, n_actions] (float32, or float64 read as
    float32); agents = [(obs0, obs_w, act0, act_w)].  Columns no agent owns stay zero, and so do the values of an agent whose value
    state dict is None."""
    obs = np.asarray(obs, dtype=F)
    act = np.asarray(actions).astype(F)
    T, N = obs.shape[0] - 1, obs.shape[1]
    out = {"values": np.zeros((T, N, len(agents)), dtype=F), "next_values": np.zeros((T, N, len(agents)), dtype=F),
           "h": np.zeros((len(agents), T, N, H), dtype=F), "c": np.zeros((len(agents), T, N, H), dtype=F)}
    for k in ("mu", "z", "std", "old_log_probs"):
        out[k] = np.zeros(act.shape, dtype=F)
    for i, ((o0, ow, a0, aw), asd, vsd) in enumerate(zip(agents, actor_sds, value_sds)):
        x = obs[:, :, o0:o0 + ow]
        if vsd is not None:
            out["values"][:, :, i] = value_head(vsd, run(vsd, x[:T]).reshape(T * N, H)).reshape(T, N)
            out["next_values"][:, :, i] = value_head(vsd, run(vsd, x[1:]).reshape(T * N, H)).reshape(T, N)
        out["h"][i], out["c"][i] = run(asd, x[:T], with_c=True)
        mu, z, std = actor_heads(asd, out["h"][i].reshape(T * N, H), min_std, max_std)
        sl = slice(a0, a0 + aw)
        out["mu"][:, :, sl], out["z"][:, :, sl], out["std"][:, :, sl] = mu.reshape(T, N, aw), z.reshape(T, N, aw), std.reshape(T, N, aw)
        out["old_log_probs"][:, :, sl] = pm.log_prob(act[:, :, sl], out["mu"][:, :, sl], out["std"][:, :, sl])
    return out


def gae_next(rewards, values, next_values, dones, gamma, lmbda):
    """td_target, adv [T, ...] float32 with the next values in an array of their own: rollout_model.td_and_gae's operations."""
    r, v, nv, dn = (np.asarray(a, dtype=F) for a in (rewards, values, next_values, dones))
    assert v.shape == r.shape == nv.shape == dn.shape
    g, _ = rm.coefficients(gamma, lmbda)
    with np.errstate(all="ignore"):
        td_target = r + ((g * nv).astype(F) * (F(1.0) - dn)).astype(F)
        td_delta = td_target - v
    assert td_target.dtype == F and td_delta.dtype == F
    return td_target, rm.gae_from_delta(td_delta, gamma, lmbda)
