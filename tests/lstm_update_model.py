"""The arithmetic contract of the recurrent PPO agents' clipped-loss epochs (pednstream_amd/csrc/pedn_lstm_grad.hpp)
restated in numpy: TEST INFRASTRUCTURE.  The forward is tests/lstm_model.py's step (section 17) with the activated gates kept; the loss'
tail, the double sums, the slabs, clip_grad_norm_, Adam and the early stop are tests/ppo_update_model.py's (section 20); the layers' backward
pieces are tests/sac_critic_model.py's (section 18).  What this file adds is back-propagation through time: per env, t descending, every
product and sum one rounded float32 operation in the order of section 21, every accumulator from +0.0.

    forward(sd, xs)                                -> dict h, c, i, f, g, o [T, N, 64] from a zero state            xs: [T, N, obs_w]
    bptt(sd, fw, dhh)                              -> a [T, N, 256]: the pre-activation gradients of the gate rows  dhh: [T, N, 64]
    agent_gradients(actor, value, xs, act, old, adv, td, groups, ...) -> per agent: raw gradients of both networks, losses, approx_kl, ...
    Epochs(agents, actor_sds, value_sds, ...)      -> the whole update with Adam state, step counts and stop flags
"""
import numpy as np

import lstm_model as lm
import ppo_update_model as um

F = np.float32
H = lm.H
TILE = um.TILE
DEFAULT_GROUPS = um.DEFAULT_GROUPS
LSTM_KEYS = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0")
ACTOR_ORDER = list(LSTM_KEYS) + ["mean_head.weight", "mean_head.bias", "std_head.weight", "std_head.bias"]
VALUE_ORDER = list(LSTM_KEYS) + ["value_head.weight", "value_head.bias"]
cm, am, pm = um.cm, um.am, um.pm


def forward(sd, xs):
    """lstm_model.step over xs [T, N, obs_w] from h = c = +0.0, with the activated gates of every step (lstm_model.gates on the same
    inputs: the step's own pre-activations)."""
    xs = np.asarray(xs, dtype=F)
    T, N = xs.shape[0], xs.shape[1]
    h = c = np.zeros((N, H), dtype=F)
    out = {k: np.empty((T, N, H), dtype=F) for k in ("h", "c", "i", "f", "g", "o")}
    for t in range(T):
        pre = lm.gates(sd, xs[t], h)
        out["i"][t], out["f"][t], out["g"][t], out["o"][t] = (lm.sigmoid(pre[:, :H]), lm.sigmoid(pre[:, H:2 * H]), lm.tanh(pre[:, 2 * H:3 * H]),
                                                              lm.sigmoid(pre[:, 3 * H:]))
        h, c = lm.step(sd, xs[t], h, c)
        out["h"][t], out["c"][t] = h, c
    return out


def bptt(sd, fw, dhh):
    """a [T, N, 256] (gate rows i, f, g, o) from dhh [T, N, 64], the gradient that reaches h'[t] from the heads behind the ReLU's mask."""
    whh = np.asarray(sd["lstm.weight_hh_l0"], dtype=F)
    T, N = fw["h"].shape[0], fw["h"].shape[1]
    one = F(1)
    dh_rec = dc_rec = np.zeros((N, H), dtype=F)
    a = np.zeros((T, N, 4 * H), dtype=F)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            i, f, g, o = (fw[k][t] for k in "ifgo")
            c_prev = fw["c"][t - 1] if t > 0 else np.zeros((N, H), dtype=F)
            tc = lm.tanh(fw["c"][t])
            dh = dhh[t] + dh_rec
            d_o = dh * tc
            dtc = dh * o
            u = one - tc * tc
            dc = dtc * u
            dc = dc + dc_rec
            d_i, d_g, d_f = dc * g, dc * i, dc * c_prev
            dc_rec = dc * f
            a[t, :, :H] = d_i * (i * (one - i))
            a[t, :, H:2 * H] = d_f * (f * (one - f))
            a[t, :, 2 * H:3 * H] = d_g * (one - g * g)
            a[t, :, 3 * H:] = d_o * (o * (one - o))
            assert dc_rec.dtype == F and dh.dtype == F
            dh_rec = cm.dx(a[t], whh, H)                  # one chain over the 256 gate rows, ascending, from +0.0
    return a


def lstm_tile(a, x, hprev, rows, g):
    g["lstm.weight_ih_l0"], g["lstm.bias_ih_l0"] = cm.dw(a[rows], x[rows])
    g["lstm.weight_hh_l0"], g["lstm.bias_hh_l0"] = cm.dw(a[rows], hprev[rows])          # (the t = 0 rows multiply +0.0 and are in the chain)
    return g


def agent_gradients(actor, value, xs, act, old, adv, td, groups=DEFAULT_GROUPS, clip_eps=0.2, min_std=1e-3, max_std=10.0, stages=None, live=None):
    """One agent; xs [T, N, obs_w], act / old [T, N, act_w], adv / td [T, N].  Rows are r = t * N + e.  stages: earlier results to use in
    place of the model's own (std, logp; d_mu, d_z), as a staged comparison feeds a kernel's outputs to the next stage.  live: the steps
    that count (R = live * N): the rows behind them are in no chain, whatever they hold."""
    if live is not None:
        xs, act, old, adv, td = (np.asarray(v)[:int(live)] for v in (xs, act, old, adv, td))
        stages = {k: np.asarray(v)[:int(live)] for k, v in stages.items()} if stages else stages
    xs = np.asarray(xs, dtype=F)
    T, N = xs.shape[0], xs.shape[1]
    R = T * N
    flat = lambda v: np.asarray(v).reshape(R, -1)
    x = flat(xs)
    afw, vfw = forward(actor, xs), forward(value, xs)
    prev = lambda fw: np.concatenate([np.zeros((1, N, H), dtype=F), fw["h"][:-1]], axis=0).reshape(R, H)
    # ---- the actor's heads and the loss' tail
    ah = am.relu(afw["h"].reshape(R, H))
    mu, z, std = lm.actor_heads(actor, afw["h"].reshape(R, H), min_std, max_std)
    t = {"mu": mu, "z": z, "sp": am.softplus(z), "std": std, "act": flat(act).astype(F)}
    t["logp"] = pm.log_prob(t["act"], mu, std)
    own = {"std": t["std"], "logp": t["logp"]}
    if stages:
        t.update({k: flat(stages[k]).astype(F) for k in ("std", "logp") if k in stages})
    d_mu, d_z, el, ek, cls = um.tail(t, flat(old), np.asarray(adv, dtype=F).reshape(R), R, clip_eps, min_std, max_std)
    own["d_mu"], own["d_z"] = d_mu, d_z
    if stages and "d_mu" in stages:
        d_mu, d_z = flat(stages["d_mu"]).astype(F), flat(stages["d_z"]).astype(F)
    wheads = np.concatenate([np.asarray(actor["mean_head.weight"], dtype=F), np.asarray(actor["std_head.weight"], dtype=F)], axis=0)
    a_act = bptt(actor, afw, cm.mask(cm.dx(np.concatenate([d_mu, d_z], axis=1), wheads, H), ah).reshape(T, N, H)).reshape(R, 4 * H)
    # ---- the value network
    vh = am.relu(vfw["h"].reshape(R, H))
    v = lm.value_head(value, vfw["h"].reshape(R, H))
    with np.errstate(all="ignore"):
        e = (v - np.asarray(td, dtype=F).reshape(R)).astype(F)
        dv = (e * F(2.0 / float(R))).astype(F)
        dvh = cm.mask((dv[:, None] * np.asarray(value["value_head.weight"], dtype=F)[0][None, :]).astype(F), vh)
    a_val = bptt(value, vfw, dvh.reshape(T, N, H)).reshape(R, 4 * H)
    ahp, vhp = prev(afw), prev(vfw)
    ga, gv, sl, sk, sq = [], [], [], [], []
    for r0 in range(0, R, TILE):
        rows = slice(r0, min(r0 + TILE, R))
        g = lstm_tile(a_act, x, ahp, rows, {})
        g["mean_head.weight"], g["mean_head.bias"] = cm.dw(d_mu[rows], ah[rows])
        g["std_head.weight"], g["std_head.bias"] = cm.dw(d_z[rows], ah[rows])
        ga.append(g)
        g = lstm_tile(a_val, x, vhp, rows, {})
        g["value_head.weight"], g["value_head.bias"] = cm.dw(dv[rows][:, None], vh[rows])
        gv.append(g)
        sl.append(um.chain64(el[rows]))
        sk.append(um.chain64(ek[rows]))
        with np.errstate(all="ignore"):
            sq.append(um.chain64x(e[rows]))
    cnt = float(R) * float(mu.shape[1])
    with np.errstate(all="ignore"):
        out = {"actor": um.reduce_groups(ga, groups), "value": um.reduce_groups(gv, groups), "actor_loss": F(um.reduce_groups(sl, groups) / cnt),
               "approx_kl": F(um.reduce_groups(sk, groups) / cnt), "critic_loss": F(um.reduce_groups(sq, groups) / float(R))}
    # rows r = t * N + e, as tests/ppo_update_model.py returns them
    out.update({"log_probs": t["logp"], "values": v, "mu": mu, "std": t["std"], "d_mu": d_mu, "d_z": d_z, "class": cls, "own": own, "el": el,
                "a_actor": a_act, "a_value": a_val, "gates": {"actor": afw, "value": vfw}})
    return out


class Epochs(um.Epochs):
    """The update of every agent: parameters (copies of the state dicts), Adam state, step counts and stop flags; section 20's class with
    this file's gradients."""

    def __init__(self, agents, actor_sds, value_sds, min_std=1e-3, max_std=10.0):
        super().__init__(agents, actor_sds, value_sds, 1, min_std, max_std)

    def gradients(self, obs, actions, old_log_probs, advantages, td_target, groups=None, clip_eps=0.2, max_grad_norm=0.5, agents=None, stages=None):
        """Per agent (None for a stopped one) agent_gradients' dict with the norms, coefficients and clipped gradients added.  obs [T + 1,
        N, n_obs]: env e is one sequence obs[0 .. T - 1][e]."""
        obs = np.asarray(obs, dtype=F)
        T = obs.shape[0] - 1
        act, old = np.asarray(actions).astype(F), np.asarray(old_log_probs, dtype=F)
        adv, td = np.asarray(advantages, dtype=F), np.asarray(td_target, dtype=F)
        res = []
        for i, (o0, ow, a0, aw) in enumerate(self.agents):
            if self.flags[i] or (agents is not None and i not in agents):
                res.append(None)
                continue
            sl = slice(a0, a0 + aw)
            r = agent_gradients(self.actor[i], self.value[i], obs[:T, :, o0:o0 + ow], act[:, :, sl], old[:, :, sl], adv[:, :, i], td[:, :, i],
                                DEFAULT_GROUPS if groups is None else groups, clip_eps, self.min_std, self.max_std,
                                stages={k: np.asarray(v, dtype=F)[:, :, sl] for k, v in stages.items()} if stages else None)
            r["actor_norm"], r["actor_coef"], r["actor_clipped"] = um.clip(r["actor"], ACTOR_ORDER, max_grad_norm)
            r["value_norm"], r["value_coef"], r["value_clipped"] = um.clip(r["value"], VALUE_ORDER, max_grad_norm)
            res.append(r)
        return res
