"""The arithmetic contract of PPO's clipped-loss epochs (pednstream_amd/csrc/pedn_ppo_grad.hpp) restated in numpy: TEST
INFRASTRUCTURE.  The forwards are tests/ppo_eval_model.py's (section 16) with the activations kept, the layers' backward pieces are
tests/sac_critic_model.py's (section 18), Adam is tests/sac_actor_model.py's (section 19).  Every float32 product and sum is one rounded
operation; every accumulator starts at +0.0; rows ascend within a tile of TILE rows; group g of G = min(tiles, groups) takes the tiles g,
g + G, ... ascending, stores the first partial and adds every later one; the groups' slabs are added from +0.0, g ascending.  The loss' tail
is evaluated in float64 from the float32 values and rounded once per result.  The three sums of
scalars (the loss' elements, logp - old, the squared value errors) run in float64 from the float32 elements, the mean rounded once.  Rows past
T * N are in no sum.

    layer_norm_keep(x, g, b)                       -> y, xh, sd: section 14's LayerNorm with what its backward needs
    layer_norm_grad(dy, xh, sd, g)                 -> dx
    actor_forward(sd, x, act, min_std, max_std)    -> dict x0, h1, h2, xh, sd, h3, mu, z, sp, std, logp
    value_forward(sd, x)                           -> dict x0, h1, h2, h3, v
    tail(fw, old, adv, R, clip_eps, ...)           -> d_mu, d_z, -min(surr1, surr2), logp - old, class (0 tie, 1 surr1, 2 surr2)
    gradients(...)                                 -> per agent: raw gradients of both networks, losses, approx_kl, forward outputs
    clip(g, order, max_norm)                       -> norm, coef, clipped
    Epochs(...)                                    -> the whole update with Adam state, step counts and stop flags
"""
import numpy as np

import actor_model as am
import ppo_eval_model as pm
import sac_actor_model as sam
import sac_critic_model as cm

F = np.float32
D = np.float64
TILE = 32
DEFAULT_GROUPS = 512
NORM_BLOCKS = 16
ACTOR_KEYS = ("encoder.fc1", "encoder.fc2", "fc", "ln", "fc_mu", "fc_std")
VALUE_KEYS = ("encoder.fc1", "encoder.fc2", "fc", "value_head")


def order(keys):
    return [k + s for k in keys for s in (".weight", ".bias")]


def layer_norm_keep(x, g, b):
    with np.errstate(all="ignore"):
        mean = am.tree_sum(x) / F(64)
        c = (x - mean[:, None]).astype(F)
        var = am.tree_sum((c * c).astype(F)) / F(64)
        sd = np.sqrt((var + F(1e-5)).astype(F)).astype(F)
        xh = (c / sd[:, None]).astype(F)
        y = ((xh * np.asarray(g, dtype=F)).astype(F) + np.asarray(b, dtype=F)).astype(F)
    return y, xh, sd


def layer_norm_grad(dy, xh, sd, g):
    """dxh = dy * g, m1 = tree(dxh) / 64, m2 = tree(dxh * xh) / 64, dx = ((dxh - m1) - xh * m2) / sd"""
    with np.errstate(all="ignore"):
        dxh = (np.asarray(dy, dtype=F) * np.asarray(g, dtype=F)).astype(F)
        m1 = am.tree_sum(dxh) / F(64)
        m2 = am.tree_sum((dxh * xh).astype(F)) / F(64)
        return (((dxh - m1[:, None]).astype(F) - (xh * m2[:, None]).astype(F)).astype(F) / sd[:, None]).astype(F)


def actor_forward(sd, x, act, min_std=1e-3, max_std=10.0):
    p = lambda k: (sd[k + ".weight"], sd[k + ".bias"])
    x0 = am.flatten_stack(x)
    h1 = am.relu(am.linear(*p("encoder.fc1"), x0))
    h2 = am.relu(am.linear(*p("encoder.fc2"), h1))
    y, xh, lsd = layer_norm_keep(am.linear(*p("fc"), h2), sd["ln.weight"], sd["ln.bias"])
    h3 = am.relu(y)
    mu, z = am.linear(*p("fc_mu"), h3), am.linear(*p("fc_std"), h3)
    sp = am.softplus(z)
    std = am.clip(sp, F(min_std), F(max_std))
    return {"x0": x0, "h1": h1, "h2": h2, "xh": xh, "sd": lsd, "h3": h3, "mu": mu, "z": z, "sp": sp, "std": std,
            "act": np.asarray(act).astype(F), "logp": pm.log_prob(np.asarray(act).astype(F), mu, std)}


def value_forward(sd, x):
    p = lambda k: (sd[k + ".weight"], sd[k + ".bias"])
    x0 = am.flatten_stack(x)
    h1 = am.relu(am.linear(*p("encoder.fc1"), x0))
    h2 = am.relu(am.linear(*p("encoder.fc2"), h1))
    h3 = am.relu(am.linear(*p("fc"), h2))
    return {"x0": x0, "h1": h1, "h2": h2, "h3": h3, "v": am.linear(*p("value_head"), h3)[:, 0]}


def tail(fw, old, adv, R, clip_eps=0.2, min_std=1e-3, max_std=10.0):
    """Per (row, action): the surrogate's forward in float32 (exp in double, rounded once) and torch's backward in double, rounded once per
    result.  adv [rows] is the agent's advantage, broadcast over its columns."""
    lp, old = np.asarray(fw["logp"], dtype=F), np.asarray(old, dtype=F)
    A = np.asarray(adv, dtype=F)[:, None]
    act_w = lp.shape[1]
    lo, hi = F(1.0 - float(clip_eps)), F(1.0 + float(clip_eps))
    with np.errstate(all="ignore"):
        dl = (lp - old).astype(F)
        lrc = np.where(dl < F(-20), F(-20), np.where(dl > F(20), F(20), dl)).astype(F)
        ratio = np.exp(lrc.astype(D)).astype(F)
        rc = np.where(ratio < lo, lo, np.where(ratio > hi, hi, ratio)).astype(F)
        s1, s2 = (ratio * A).astype(F), (rc * A).astype(F)
        el = (-np.where((s2 < s1) | (s2 != s2), s2, s1)).astype(F)
        w1 = np.where(s1 > s2, 0.0, np.where(s1 == s2, 0.5, 1.0))
        w2 = np.where(s1 < s2, 0.0, np.where(s1 == s2, 0.5, 1.0))
        G = -1.0 / (float(R) * float(act_w))
        pr = ((ratio >= lo) & (ratio <= hi)).astype(D)
        pl = ((dl >= F(-20)) & (dl <= F(20))).astype(D)
        dlp = (G * A.astype(D) * (w1 + w2 * pr)) * ratio.astype(D) * pl
        mu, S, a, z = (np.asarray(fw[k], dtype=F).astype(D) for k in ("mu", "std", "act", "z"))
        dm = a - mu
        d_mu = (dlp * dm / (S * S)).astype(F)
        gsd = dlp * (dm * dm / (S * S * S) - 1.0 / S)
        sp = np.asarray(fw["sp"], dtype=F)
        ps = ((sp >= F(min_std)) & (sp <= F(max_std))).astype(D)
        sg = np.where(np.asarray(fw["z"], dtype=F) > 20, 1.0, 1.0 / (1.0 + np.exp(-z)))
        d_z = (gsd * ps * sg).astype(F)
        inside = (ratio >= lo) & (ratio <= hi)
        cls = np.where(inside, 0, np.where(s1 < s2, 1, 2))
    return d_mu, d_z, el, dl, cls


def chain(v):
    return sam.chain(np.asarray(v, dtype=F).reshape(-1))


def chain64(v):
    """((0 + v_0) + v_1) + ... in float64 from the float32 elements: the sums of the loss' elements, of logp - old and of the squared errors
    cancel or are compared with a torch mean that does not sum in one chain; as float32 chains they alone carried the forward's error"""
    s = D(0)
    with np.errstate(all="ignore"):
        for x in np.asarray(v, dtype=F).reshape(-1).astype(D):
            s = D(s + x)
    return s


def chain64x(e):
    """the chain of e * e in float64 (a float32 square is exact there)"""
    s = D(0)
    for x in np.asarray(e, dtype=F).astype(D):
        s = D(s + x * x)
    return s


def actor_tile(sd, fw, d_mu, d_z, r0, r1):
    rows = slice(r0, r1)
    w = lambda k: np.asarray(sd[k + ".weight"], dtype=F)
    dmu, dz = d_mu[rows], d_z[rows]
    g = {}
    g["fc_mu.weight"], g["fc_mu.bias"] = cm.dw(dmu, fw["h3"][rows])
    g["fc_std.weight"], g["fc_std.bias"] = cm.dw(dz, fw["h3"][rows])
    dy = cm.mask(cm.dx(np.concatenate([dmu, dz], axis=1), np.concatenate([w("fc_mu"), w("fc_std")], axis=0), 64), fw["h3"][rows])
    with np.errstate(all="ignore"):
        gw = np.zeros(64, dtype=F)
        gb = np.zeros(64, dtype=F)
        for r in range(dy.shape[0]):
            gw = (gw + (dy[r] * fw["xh"][rows][r]).astype(F)).astype(F)
            gb = (gb + dy[r]).astype(F)
    g["ln.weight"], g["ln.bias"] = gw, gb
    d3 = layer_norm_grad(dy, fw["xh"][rows], fw["sd"][rows], sd["ln.weight"])
    return trunk_tile(sd, fw, d3, rows, g)


def trunk_tile(sd, fw, d3, rows, g):
    w = lambda k: np.asarray(sd[k + ".weight"], dtype=F)
    g["fc.weight"], g["fc.bias"] = cm.dw(d3, fw["h2"][rows])
    d2 = cm.mask(cm.dx(d3, w("fc"), 64), fw["h2"][rows])
    g["encoder.fc2.weight"], g["encoder.fc2.bias"] = cm.dw(d2, fw["h1"][rows])
    d1 = cm.mask(cm.dx(d2, w("encoder.fc2"), 64), fw["h1"][rows])
    g["encoder.fc1.weight"], g["encoder.fc1.bias"] = cm.dw(d1, fw["x0"][rows])
    return g


def value_tile(sd, fw, dv, r0, r1):
    rows = slice(r0, r1)
    g = {}
    gw, gb = cm.dw(dv[rows][:, None], fw["h3"][rows])
    g["value_head.weight"], g["value_head.bias"] = gw, gb
    with np.errstate(all="ignore"):
        d3 = cm.mask((dv[rows][:, None] * np.asarray(sd["value_head.weight"], dtype=F)[0][None, :]).astype(F), fw["h3"][rows])
    return trunk_tile(sd, fw, d3, rows, g)


def reduce_groups(partials, groups):
    """partials: per tile a dict (or a float32 scalar); group g adds tiles g, g + G, ... to its first; the slabs are added from +0.0."""
    G = min(len(partials), int(groups))
    add = lambda a, b: {k: (a[k] + b[k]).astype(F) for k in a} if isinstance(a, dict) else type(a)(a + b)
    total = None
    with np.errstate(all="ignore"):
        for g in range(G):
            slab = partials[g]
            for t in range(g + G, len(partials), G):
                slab = add(slab, partials[t])
            if total is None:
                total = {k: np.zeros_like(v) for k, v in slab.items()} if isinstance(slab, dict) else type(slab)(0)
            total = add(total, slab)
    return total


def agent_gradients(actor, value, x, act, old, adv, td, groups=DEFAULT_GROUPS, clip_eps=0.2, min_std=1e-3, max_std=10.0, live=None, stages=None):
    """One agent, x [R, S, obs_w] (rows behind `live` are in no sum): the unclipped gradients of both networks and the scalars.  stages:
    earlier results to use in place of the model's own (std, logp; d_mu, d_z), as a staged comparison feeds a kernel's outputs to the
    next stage."""
    R = x.shape[0] if live is None else int(live)
    afw, vfw = actor_forward(actor, x, act, min_std, max_std), value_forward(value, x)
    own = {"std": afw["std"], "logp": afw["logp"]}
    if stages:
        afw.update({k: np.asarray(stages[k], dtype=F) for k in ("std", "logp") if k in stages})
    d_mu, d_z, el, ek, cls = tail(afw, old, adv, R, clip_eps, min_std, max_std)
    own["d_mu"], own["d_z"] = d_mu, d_z
    if stages and "d_mu" in stages:
        d_mu, d_z = np.asarray(stages["d_mu"], dtype=F), np.asarray(stages["d_z"], dtype=F)
    with np.errstate(all="ignore"):
        e = (vfw["v"] - np.asarray(td, dtype=F)).astype(F)
        dv = (e * F(2.0 / float(R))).astype(F)
    ga, gv, sl, sk, sq = [], [], [], [], []
    for r0 in range(0, R, TILE):
        r1 = min(r0 + TILE, R)
        ga.append(actor_tile(actor, afw, d_mu, d_z, r0, r1))
        gv.append(value_tile(value, vfw, dv, r0, r1))
        sl.append(chain64(el[r0:r1]))
        sk.append(chain64(ek[r0:r1]))
        with np.errstate(all="ignore"):
            sq.append(chain64x(e[r0:r1]))
    act_w = afw["mu"].shape[1]
    cnt = float(R) * float(act_w)
    with np.errstate(all="ignore"):
        out = {"actor": reduce_groups(ga, groups), "value": reduce_groups(gv, groups), "actor_loss": F(reduce_groups(sl, groups) / cnt),
               "approx_kl": F(reduce_groups(sk, groups) / cnt), "critic_loss": F(reduce_groups(sq, groups) / float(R))}
    out.update({"log_probs": afw["logp"], "values": vfw["v"], "mu": afw["mu"], "std": afw["std"], "d_mu": d_mu, "d_z": d_z, "class": cls,
                "own": own, "el": el})
    return out


def sum_squares(g, keys):
    """sum g^2 in float64 in the order of ppograd_reduce_kernel: the network's elements in the pack's order, element i on thread i mod
    (16 * 256); a thread's elements ascending, a halving tree over the 256 threads of a workgroup, the 16 workgroups ascending."""
    flat = np.concatenate([np.asarray(g[k], dtype=F).reshape(-1) for k in keys]).astype(D)
    n = NORM_BLOCKS * 256
    pad = np.zeros(-(-flat.size // n) * n, dtype=D)
    pad[:flat.size] = flat
    sq = (pad * pad).reshape(-1, NORM_BLOCKS, 256)
    with np.errstate(all="ignore"):
        acc = np.zeros((NORM_BLOCKS, 256), dtype=D)
        for k in range(sq.shape[0]):
            acc = acc + sq[k]
        h = 128
        while h:
            acc = acc[:, :h] + acc[:, h:2 * h]
            h //= 2
        total = D(0)
        for b in range(NORM_BLOCKS):
            total = total + acc[b, 0]
    return total


def clip(g, keys, max_norm=0.5):
    """clip_grad_norm_: (total_norm, coef, the clipped gradients): coef = min(max_norm / (total_norm + 1e-6), 1) in float32, g = g * coef."""
    with np.errstate(all="ignore"):
        norm = F(np.sqrt(sum_squares(g, keys)))
        coef = F(F(max_norm) / F(norm + F(1e-6)))
        coef = F(1) if coef > 1 else coef
        return norm, coef, {k: (np.asarray(g[k], dtype=F) * coef).astype(F) for k in keys}


class Epochs:
    """The update of every agent: parameters (copies of the state dicts), Adam state, step counts and stop flags."""

    def __init__(self, agents, actor_sds, value_sds, S, min_std=1e-3, max_std=10.0):
        self.agents, self.S, self.min_std, self.max_std = [tuple(a) for a in agents], int(S), min_std, max_std
        cp = lambda sd: {k: np.array(v, dtype=F) for k, v in sd.items()}
        self.actor, self.value = [cp(sd) for sd in actor_sds], [cp(sd) for sd in value_sds]
        zeros = lambda sds: [{k: np.zeros_like(v) for k, v in sd.items()} for sd in sds]
        self.m = {"actor": zeros(self.actor), "value": zeros(self.value)}
        self.v = {"actor": zeros(self.actor), "value": zeros(self.value)}
        self.steps, self.flags, self.last = [0] * len(agents), [0] * len(agents), [None] * len(agents)

    def begin_update(self):
        self.flags = [0] * len(self.agents)

    def gradients(self, obs, actions, old_log_probs, advantages, td_target, groups=None, clip_eps=0.2, max_grad_norm=0.5, agents=None, stages=None):
        """Per agent (None for a stopped one) agent_gradients' dict with the norms, coefficients and clipped gradients added."""
        obs = np.asarray(obs, dtype=F)
        T, N = obs.shape[0] - 1, obs.shape[1]
        R = T * N
        st = pm.stacks(obs, self.S)[:T].reshape(R, self.S, obs.shape[2])
        act = np.asarray(actions).astype(F).reshape(R, -1)
        old = np.asarray(old_log_probs, dtype=F).reshape(R, -1)
        adv, td = np.asarray(advantages, dtype=F).reshape(R, -1), np.asarray(td_target, dtype=F).reshape(R, -1)
        res = []
        for i, (o0, ow, a0, aw) in enumerate(self.agents):
            if self.flags[i] or (agents is not None and i not in agents):
                res.append(None)
                continue
            sl = slice(a0, a0 + aw)
            r = agent_gradients(self.actor[i], self.value[i], st[:, :, o0:o0 + ow], act[:, sl], old[:, sl], adv[:, i], td[:, i],
                                DEFAULT_GROUPS if groups is None else groups, clip_eps, self.min_std, self.max_std,
                                stages={k: np.asarray(v, dtype=F).reshape(R, -1)[:, sl] for k, v in stages.items()} if stages else None)
            r["actor_norm"], r["actor_coef"], r["actor_clipped"] = clip(r["actor"], order(ACTOR_KEYS), max_grad_norm)
            r["value_norm"], r["value_coef"], r["value_clipped"] = clip(r["value"], order(VALUE_KEYS), max_grad_norm)
            res.append(r)
        return res

    def epoch_update(self, obs, actions, old_log_probs, advantages, td_target, actor_lr=3e-4, critic_lr=6e-4, clip_eps=0.2, max_grad_norm=0.5,
                     kl_tolerance=0.01, betas=(0.9, 0.999), eps=1e-8, groups=None, agents=None, stages=None):
        res = self.gradients(obs, actions, old_log_probs, advantages, td_target, groups, clip_eps, max_grad_norm, agents, stages)
        for i, r in enumerate(res):
            if r is None:
                continue
            self.steps[i] += 1
            for name, params, lr in (("actor", self.actor[i], actor_lr), ("value", self.value[i], critic_lr)):
                for k in params:
                    params[k], self.m[name][i][k], self.v[name][i][k] = sam.adam(params[k], r[name + "_clipped"][k], self.m[name][i][k],
                                                                                 self.v[name][i][k], self.steps[i], lr, betas, eps)
            if float(r["approx_kl"]) > 1.5 * float(kl_tolerance):
                self.flags[i] = 1
            self.last[i] = r
        return res
