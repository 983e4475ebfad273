"""The rollout contract restated in numpy -- what pednstream_amd/csrc/pedn_rollout.hpp must compute bit for bit, the
way tests/norm_model.py restates the running normalisation.  TD targets and GAE: IEEE binary32 + - * on arrays, one operation and one
rounding at a time; the advantage normalisation: binary64 with the fixed summation order S of norm_model.fixed_sum over the env axis.

    td_target, adv = td_and_gae(rewards, values, dones, gamma, lmbda)      # [T, ...], [T + 1, ...], [T, ...] float32
    adv = gae_from_delta(td_delta, gamma, lmbda)                           # the reference's compute_gae on [T, ...]
    adv_n = normalize_advantages(adv)                                      # [T, n_envs, n_agents] float32 -> float32
"""
import numpy as np

from norm_model import fixed_sum

F = np.float32


def coefficients(gamma, lmbda):
    """(g, c): gamma rounded once to binary32; gamma * lmbda taken in binary64 and rounded once."""
    return F(float(gamma)), F(float(gamma) * float(lmbda))


def gae_from_delta(td_delta, gamma, lmbda):
    d = np.asarray(td_delta, dtype=F)
    _, c = coefficients(gamma, lmbda)
    adv = np.empty_like(d)
    carry = np.zeros(d.shape[1:], dtype=F)                # +0.0; NOT masked by done
    with np.errstate(all="ignore"):
        for t in range(d.shape[0] - 1, -1, -1):
            carry = (c * carry).astype(F) + d[t]
            adv[t] = carry
    return adv


def td_and_gae(rewards, values, dones, gamma, lmbda):
    r, v, dn = np.asarray(rewards, dtype=F), np.asarray(values, dtype=F), np.asarray(dones, dtype=F)
    assert v.shape == (r.shape[0] + 1,) + r.shape[1:] and dn.shape == r.shape
    g, _ = coefficients(gamma, lmbda)
    with np.errstate(all="ignore"):
        td_target = r + ((g * v[1:]).astype(F) * (F(1.0) - dn)).astype(F)
        td_delta = td_target - v[:-1]
    assert td_target.dtype == F and td_delta.dtype == F
    return td_target, gae_from_delta(td_delta, gamma, lmbda)


def normalize_advantages(adv):
    """Per agent over all T * n_envs entries: (x - mean) / (std + 1e-8), torch's unbiased std, in binary64, rounded to float32."""
    x = np.asarray(adv, dtype=F).astype(np.float64)
    T, N, A = x.shape
    n = float(T) * float(N)
    if T * N < 2:
        raise ValueError("advantage normalisation needs at least two entries per agent")

    def total(y):                                        # S over the env axis of every time row, the T row sums in increasing t
        rows = fixed_sum(y.transpose(1, 0, 2))           # [T, A]
        tot = rows[0].copy()
        for t in range(1, T):
            tot = tot + rows[t]
        return tot

    mean = total(x) / n
    d = x - mean
    std = np.sqrt(total(d * d) / (n - 1.0))
    return ((x - mean) / (std + 1e-8)).astype(F)
