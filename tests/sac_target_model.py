"""The arithmetic contract of the SAC TD targets and the Polyak update (pednstream_amd/csrc/pedn_sac.hpp) restated in
numpy: TEST INFRASTRUCTURE.  The actor and the layers are those of tests/actor_model.py (section 14); every float32 product and sum is one
rounded operation; the squashing and the log-probability are evaluated in float64 from the float32 values and rounded once.

    noise(seed, b, c, d)                         -> eps float32 of row b, whole-row action column c, draw d (stream 0x73)
    tail(mu, std, eps, max_delta)                -> u, t, next_action, logp  float32 [B, act_w]
    entropy(logp)                                -> float32 [B]
    critic(sd, x, next_action)                   -> q float32 [B]        x: [B, S, obs_w]
    td(q1, q2, entropy, log_alpha, r, done, gamma) -> float32 [B]
    target(actor_sd, c1_sd, c2_sd, x, r, done, eps, log_alpha, gamma, max_delta) -> dict of every output of one agent
    polyak(target, online, tau)                  -> float32
"""
import math

import numpy as np

import actor_model as am

F = np.float32
NOISE_SITE = 0x73
LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
CRITIC_KEYS = ("encoder.fc1", "encoder.fc2", "fc", "fc_out")


def noise(seed, b, c, d):
    """eps of row b, action column c, draw d: section 14's Box-Muller on the stream of tag 0x73."""
    b, c, d = (np.asarray(v, dtype=np.uint64) for v in (b, c, d))
    mask = np.uint64(0xFFFFFFFF)
    w = am.philox4x32_10((b, d & mask, np.uint64(NOISE_SITE) | (c << np.uint64(8)), d >> np.uint64(32)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1 = (w[0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = w[1].astype(np.float64) * 2.0 ** -32
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(F)


def squash(mu, std, eps, max_delta=2.5):
    """u = mu + std * eps, t = tanh(u), next_action = t * max_delta: float32 each."""
    mu, std, eps = (np.asarray(v, dtype=F) for v in (mu, std, eps))
    with np.errstate(all="ignore"):
        u = (mu + (std * eps).astype(F)).astype(F)
        t = np.tanh(u.astype(np.float64)).astype(F)
        return u, t, (t * F(max_delta)).astype(F)


def log_prob(u, mu, std, t):
    """Normal(mu, std).log_prob(u) - log(1 - tanh(t)^2 + 1e-7) in float64 from the float32 values, rounded once.  The reference applies
    tanh to the already squashed action t (SAC.py:302); this is mirrored."""
    U, M, S, T = (np.asarray(v, dtype=F).astype(np.float64) for v in (u, mu, std, t))
    with np.errstate(all="ignore"):
        th = np.tanh(T)
        return (-((U - M) * (U - M)) / (2.0 * (S * S)) - np.log(S) - LOG_SQRT_2PI - np.log(1.0 - th * th + 1e-7)).astype(F)


def tail(mu, std, eps, max_delta=2.5):
    u, t, na = squash(mu, std, eps, max_delta)
    return u, t, na, log_prob(u, mu, std, t)


def entropy(logp):
    """((0 - logp_0) - logp_1) - ..., ascending, float32."""
    logp = np.asarray(logp, dtype=F)
    ent = np.zeros(logp.shape[0], dtype=F)
    with np.errstate(all="ignore"):
        for j in range(logp.shape[1]):
            ent = (ent - logp[:, j]).astype(F)
    return ent


def critic(sd, x, next_action):
    """q [B] of the critic whose state dict (reference keys, arrays) is sd: feat = [encoder (64), next_action (act_w), the newest frame's
    last column]; no ReLU between fc and fc_out."""
    x = np.asarray(x, dtype=F)
    p = lambda k: (sd[k + ".weight"], sd[k + ".bias"])
    zs = am.relu(am.linear(*p("encoder.fc1"), am.flatten_stack(x)))
    zs = am.relu(am.linear(*p("encoder.fc2"), zs))
    feat = np.concatenate([zs, np.asarray(next_action, dtype=F), x[:, -1, -1:]], axis=1).astype(F)
    h = am.linear(*p("fc"), feat)
    return am.linear(*p("fc_out"), h)[:, 0]


def q_min(q1, q2):
    """torch.min: the smaller one, NaN wins."""
    q1, q2 = np.asarray(q1, dtype=F), np.asarray(q2, dtype=F)
    with np.errstate(invalid="ignore"):
        return np.where((q2 < q1) | (q2 != q2), q2, q1).astype(F)


def td(q1, q2, ent, log_alpha, rewards, dones, gamma=0.99):
    alpha = F(np.exp(np.float64(F(log_alpha))))
    with np.errstate(all="ignore"):
        nv = (q_min(q1, q2) + (alpha * np.asarray(ent, dtype=F)).astype(F)).astype(F)
        return (np.asarray(rewards, dtype=F) + ((F(gamma) * nv).astype(F) * (F(1) - np.asarray(dones, dtype=F))).astype(F)).astype(F)


def target(actor_sd, c1_sd, c2_sd, x, rewards, dones, eps, log_alpha, gamma=0.99, max_delta=2.5):
    """Every output of one agent for its columns x [B, S, obs_w], rewards [B], dones [B], eps [B, act_w]."""
    mu, z, std = am.forward("sac", actor_sd, x)
    u, t, na, logp = tail(mu, std, eps, max_delta)
    ent = entropy(logp)
    q1, q2 = critic(c1_sd, x, na), critic(c2_sd, x, na)
    return {"mu": mu, "std": std, "eps": np.asarray(eps, dtype=F), "u": u, "t": t, "logp": logp, "next_actions": na, "entropy": ent, "q1": q1, "q2": q2,
            "td_target": td(q1, q2, ent, log_alpha, rewards, dones, gamma)}


def polyak(target_values, online_values, tau):
    """target * (float)(1 - tau) + online * (float)tau, 1 - tau formed in double."""
    t, o = np.asarray(target_values, dtype=F), np.asarray(online_values, dtype=F)
    with np.errstate(all="ignore"):
        return ((t * F(1.0 - float(tau))).astype(F) + (o * F(float(tau))).astype(F)).astype(F)
