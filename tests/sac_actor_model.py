"""The arithmetic contract of the SAC actor and temperature step (pednstream_amd/csrc/pedn_actor_grad.hpp) restated in
numpy: TEST INFRASTRUCTURE.  The actor's forward is tests/actor_model.py's (section 14), the tail and the critics are
tests/sac_target_model.py's (section 15), the layers' backward pieces are tests/sac_critic_model.py's (section 18), Adam is section 18's with
exp_avg_sq's multiply-add fused.  Every float32
product and sum is one rounded operation; every accumulator starts at +0.0; rows ascend within a tile of TILE rows, tiles ascend, output
neurons ascend in an input gradient.  The per-(row, action) tail of the backward is evaluated in float64 from the float32 values and rounded
once, like the forward's tail.  Rows past B are in no sum.

    noise(seed, b, c, d)                          -> eps float32 of row b, whole-row action column c, draw d (stream 0x75)
    forward(actor, c1, c2, x, eps, max_delta)     -> dict x0, h1, h2, h3, mu, z, std, eps, u, t, new_actions, logp, entropy, q1, q2
    dq_daction(critic, act_w)                     -> float64 [act_w]: sum over o ascending of fc_out[o] * fc[o][64 + j]
    min_weights(q1, q2)                           -> w1, w2 float64 [B]: torch.minimum's backward
    head_gradients(fw, v1, v2, log_alpha, B, max_delta) -> d_mu, d_z float32 [B, act_w]
    row_terms(fw, log_alpha, target_entropy)      -> (-alpha * entropy - min_q, entropy - target_entropy) float32 [B]
    tile_gradients(actor, fw, d_mu, d_z, r0, r1)  -> {key: partial gradient} of rows [r0, r1)
    adam(p, g, m, v, t, lr, betas, eps)           -> p, m, v behind step t (1-based): section 18's, v = fma((1 - b2) g, g, v b2)
    gradients(actor, c1, c2, x, eps, log_alpha, target_entropy, max_delta, tile=TILE, stages=None)
                                                  -> ({key: gradient}, {actor_loss, alpha_loss, alpha_grad}, fw)
"""
import numpy as np

import actor_model as am
import sac_critic_model as cm
import sac_target_model as sm

F = np.float32
D = np.float64
TILE = 32
NOISE_SITE = 0x75
KEYS = ("encoder.fc1", "encoder.fc2", "fc", "fc_mu", "fc_std")


def noise(seed, b, c, d):
    """eps of row b, action column c, draw d: section 14's Box-Muller on the stream of tag 0x75."""
    b, c, d = (np.asarray(v, dtype=np.uint64) for v in (b, c, d))
    mask = np.uint64(0xFFFFFFFF)
    w = am.philox4x32_10((b, d & mask, np.uint64(NOISE_SITE) | (c << np.uint64(8)), d >> np.uint64(32)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1 = (w[0].astype(D) + 1.0) * 2.0 ** -32
    u2 = w[1].astype(D) * 2.0 ** -32
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).astype(F)


def forward(actor, c1, c2, x, eps, max_delta=2.5):
    """The actor with its activations kept, section 15's tail and both critics on (x, new_actions)."""
    x = np.asarray(x, dtype=F)
    p = lambda k: (actor[k + ".weight"], actor[k + ".bias"])
    x0 = am.flatten_stack(x)
    h1 = am.relu(am.linear(*p("encoder.fc1"), x0))
    h2 = am.relu(am.linear(*p("encoder.fc2"), h1))
    h3 = am.relu(am.linear(*p("fc"), h2))
    mu, z = am.linear(*p("fc_mu"), h3), am.linear(*p("fc_std"), h3)
    std = am.softplus(z)
    u, t, na, logp = sm.tail(mu, std, eps, max_delta)
    return {"x0": x0, "h1": h1, "h2": h2, "h3": h3, "mu": mu, "z": z, "std": std, "eps": np.asarray(eps, dtype=F), "u": u, "t": t, "new_actions": na,
            "logp": logp, "entropy": sm.entropy(logp), "q1": sm.critic(c1, x, na), "q2": sm.critic(c2, x, na)}


def dq_daction(critic, act_w):
    """A critic is linear behind its encoder: d q / d action_j does not depend on the row.  float64 from the float32 weights, o ascending
    from +0.0, and handed to the tail as it is: the 64 terms cancel, and as a float32 chain this sum alone carried the gradient's error
    (4.4 times the reference's in one recorded update, 0.93 at most so)."""
    wo, w = np.asarray(critic["fc_out.weight"], dtype=F)[0].astype(D), np.asarray(critic["fc.weight"], dtype=F).astype(D)
    v = np.zeros(act_w, dtype=D)
    with np.errstate(all="ignore"):
        for o in range(w.shape[0]):
            v = v + wo[o] * w[o, 64:64 + act_w]
    assert v.dtype == D
    return v


def min_weights(q1, q2):
    """torch.minimum's backward: the smaller one takes the gradient, equal ones half each, and both all of it beside a NaN."""
    q1, q2 = np.asarray(q1, dtype=F), np.asarray(q2, dtype=F)
    with np.errstate(invalid="ignore"):
        return np.where(q1 > q2, 0.0, np.where(q1 == q2, 0.5, 1.0)), np.where(q1 < q2, 0.0, np.where(q1 == q2, 0.5, 1.0))


def alpha_of(log_alpha):
    return F(np.exp(D(F(log_alpha))))


def head_gradients(fw, v1, v2, log_alpha, B, max_delta=2.5):
    """d actor_loss / d mu and / d z of every (row, action), from the float32 t, std, eps, z, q1, q2 and the critics' float64 vectors, in float64,
    rounded once.  Normal's log-probability reaches mu through u and directly with opposite signs: folded to 0; it reaches std through u
    and directly as -eps^2 / std + eps^2 / std - 1 / std: folded to -1 / std.  softplus' derivative is torch's: 1 where z > 20."""
    w1, w2 = min_weights(fw["q1"], fw["q2"])
    t, std, eps, z = (np.asarray(fw[k], dtype=F).astype(D) for k in ("t", "std", "eps", "z"))
    with np.errstate(all="ignore"):
        G = 1.0 / float(B)
        dqa = w1[:, None] * np.asarray(v1, dtype=D)[None, :] + w2[:, None] * np.asarray(v2, dtype=D)[None, :]
        Dt = 1.0 - t * t
        T = np.tanh(t)
        omT = 1.0 - T * T
        dlp = D(alpha_of(log_alpha)) * G
        gu = (dlp * (2.0 * T * omT / (omT + 1e-7)) - G * dqa * D(F(max_delta))) * Dt
        gsd = gu * eps - dlp / std
        sp = np.where(np.asarray(fw["z"], dtype=F) > 20, 1.0, 1.0 / (1.0 + np.exp(-z)))
        return gu.astype(F), (gsd * sp).astype(F)


def fma(a, b, c):
    """float32 a * b + c with ONE rounding.  The product of two float32 is exact in float64, and so is all of the sum but its last
    rounding; rounding that to float32 again is the one rounding wanted unless the float64 sum lies exactly half way between two float32,
    where the exact sum decides (rare; evaluated in rationals)."""
    from fractions import Fraction

    a, b, c = (np.asarray(v, dtype=F) for v in np.broadcast_arrays(a, b, c))
    shape = a.shape
    a, b, c = (np.atleast_1d(v) for v in (a, b, c))
    with np.errstate(all="ignore"):
        r = a.astype(D) * b.astype(D) + c.astype(D)
        out = np.array(r.astype(F))
        lo_, hi_ = np.nextafter(out, F(-np.inf)).astype(D), np.nextafter(out, F(np.inf)).astype(D)      # (the spacing differs on the two sides of a power of 2)
        half = np.isfinite(r) & np.isfinite(lo_) & np.isfinite(hi_) & ((r == 0.5 * (lo_ + out.astype(D))) | (r == 0.5 * (hi_ + out.astype(D))))
    for i in zip(*np.nonzero(half)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = float(lo_[i]), float(hi_[i])
        out[i] = min((out[i], F(lo), F(hi)), key=lambda x: abs(Fraction(float(x)) - exact))      # (out first: an exact tie is r's own, to even)
    return out.reshape(shape)


def adam(p, g, m, v, t, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
    """Section 18's step (sac_critic_model.adam) with exp_avg_sq's last product fused into its sum: v = fma((1 - b2) g, g, v b2).  torch's
    own step fuses it; with every product rounded, one element of a recorded update lay 1.26 ulp from the float64 step where the reference
    lay 0.26, 4.83 times as far."""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    nstep, s = cm.adam_scalars(t, lr, betas)
    b2, omb1, omb2 = F(betas[1]), F(1.0 - float(betas[0])), F(1.0 - float(betas[1]))
    with np.errstate(all="ignore"):
        m = (m + (omb1 * (g - m).astype(F)).astype(F)).astype(F)
        v = fma((omb2 * g).astype(F), g, (v * b2).astype(F))
        den = ((np.sqrt(v).astype(F) / F(s)).astype(F) + F(eps)).astype(F)
        p = (p + ((F(nstep) * m).astype(F) / den).astype(F)).astype(F)
    return p, m, v


def row_terms(fw, log_alpha, target_entropy):
    alpha = alpha_of(log_alpha)
    with np.errstate(all="ignore"):
        ent = np.asarray(fw["entropy"], dtype=F)
        loss = (-(alpha * ent).astype(F) - sm.q_min(fw["q1"], fw["q2"])).astype(F)
        return loss, (ent - F(target_entropy)).astype(F)


def chain(v):
    """((0 + v_0) + v_1) + ..., float32"""
    s = F(0)
    with np.errstate(all="ignore"):
        for x in np.asarray(v, dtype=F):
            s = F(s + x)
    return s


def tile_gradients(actor, fw, d_mu, d_z, r0, r1):
    rows = slice(r0, r1)
    w = lambda k: np.asarray(actor[k + ".weight"], dtype=F)
    dmu, dz = np.asarray(d_mu, dtype=F)[rows], np.asarray(d_z, dtype=F)[rows]
    g = {}
    g["fc_mu.weight"], g["fc_mu.bias"] = cm.dw(dmu, fw["h3"][rows])
    g["fc_std.weight"], g["fc_std.bias"] = cm.dw(dz, fw["h3"][rows])
    # the two heads as one layer of 2 * act_w rows: fc_mu's first
    d3 = cm.mask(cm.dx(np.concatenate([dmu, dz], axis=1), np.concatenate([w("fc_mu"), w("fc_std")], axis=0), 64), fw["h3"][rows])
    g["fc.weight"], g["fc.bias"] = cm.dw(d3, fw["h2"][rows])
    d2 = cm.mask(cm.dx(d3, w("fc"), 64), fw["h2"][rows])
    g["encoder.fc2.weight"], g["encoder.fc2.bias"] = cm.dw(d2, fw["h1"][rows])
    d1 = cm.mask(cm.dx(d2, w("encoder.fc2"), 64), fw["h1"][rows])
    g["encoder.fc1.weight"], g["encoder.fc1.bias"] = cm.dw(d1, fw["x0"][rows])
    return g


def gradients(actor, c1, c2, x, eps, log_alpha, target_entropy, max_delta=2.5, tile=TILE, stages=None):
    """({key: gradient of actor_loss}, the three scalars, the forward) of one agent.  stages: earlier results to use in place of the
    model's own (keys of the forward, d_mu, d_z), as a staged comparison feeds a kernel's outputs to the next stage."""
    fw = forward(actor, c1, c2, x, eps, max_delta)
    if stages:
        fw.update({k: np.asarray(v, dtype=F) for k, v in stages.items() if k in fw})
    B = fw["mu"].shape[0]
    act_w = fw["mu"].shape[1]
    d_mu, d_z = head_gradients(fw, dq_daction(c1, act_w), dq_daction(c2, act_w), log_alpha, B, max_delta)
    if stages and "d_mu" in stages:
        d_mu, d_z = np.asarray(stages["d_mu"], dtype=F), np.asarray(stages["d_z"], dtype=F)
    fw["d_mu"], fw["d_z"] = d_mu, d_z
    loss, ediff = row_terms(fw, log_alpha, target_entropy)
    total, sl, se = None, F(0), F(0)
    with np.errstate(all="ignore"):
        for r0 in range(0, B, tile):
            r1 = min(r0 + tile, B)
            g = tile_gradients(actor, fw, d_mu, d_z, r0, r1)
            total = {k: (np.zeros_like(v) + v).astype(F) for k, v in g.items()} if total is None else {k: (total[k] + v).astype(F) for k, v in g.items()}
            sl, se = F(sl + chain(loss[r0:r1])), F(se + chain(ediff[r0:r1]))
        ga = F(alpha_of(log_alpha) * F(se / F(B)))
    return total, {"actor_loss": F(sl / F(B)), "alpha_loss": ga, "alpha_grad": ga}, fw
