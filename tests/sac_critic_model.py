"""The arithmetic contract of the SAC critic step (pednstream_amd/csrc/pedn_critic.hpp) restated in numpy: TEST
INFRASTRUCTURE.  The forward is tests/sac_target_model.py's critic (section 15) with the activations kept; every float32 product and sum
is one rounded operation; every accumulator starts at +0.0; rows ascend within a tile of TILE rows, tiles ascend, output neurons ascend in
an input gradient.  Rows past B are in no sum.

    forward(sd, x, actions)                  -> dict x0, h1, feat, h3, q         x: [B, S, obs_w], actions: [B, act_w]
    tile_gradients(sd, fw, td, B, r0, r1)    -> ({key: partial gradient}, partial sum of squares) of rows [r0, r1)
    gradients(sd, x, actions, td, tile=TILE) -> ({key: gradient}, loss, q)        one critic, td: [B]
    adam(p, g, m, v, t, lr, betas, eps)      -> p, m, v behind step t (1-based)   float32 arrays of one shape
    adam_scalars(t, lr, betas)               -> (-step, s) float32: the two numbers the contract evaluates in double
"""
import numpy as np

import actor_model as am

F = np.float32
TILE = 32
KEYS = ("encoder.fc1", "encoder.fc2", "fc", "fc_out")


def forward(sd, x, actions):
    x = np.asarray(x, dtype=F)
    p = lambda k: (sd[k + ".weight"], sd[k + ".bias"])
    x0 = am.flatten_stack(x)
    h1 = am.relu(am.linear(*p("encoder.fc1"), x0))
    zs = am.relu(am.linear(*p("encoder.fc2"), h1))
    feat = np.concatenate([zs, np.asarray(actions, dtype=F), x[:, -1, -1:]], axis=1).astype(F)
    h3 = am.linear(*p("fc"), feat)
    return {"x0": x0, "h1": h1, "feat": feat, "h3": h3, "q": am.linear(*p("fc_out"), h3)[:, 0]}


def dw(d, x):
    """(dW [out, in], db [out]) of rows d [R, out], x [R, in]: from +0.0, rows ascending."""
    gw, gb = np.zeros((d.shape[1], x.shape[1]), dtype=F), np.zeros(d.shape[1], dtype=F)
    with np.errstate(all="ignore"):
        for r in range(d.shape[0]):
            gw = gw + d[r][:, None] * x[r][None, :]
            gb = gb + d[r]
    assert gw.dtype == F and gb.dtype == F
    return gw, gb


def dx(d, w, cols):
    """dX [R, cols] = sum over o ascending of d[r][o] * w[o][k], from +0.0."""
    acc = np.zeros((d.shape[0], cols), dtype=F)
    with np.errstate(all="ignore"):
        for o in range(w.shape[0]):
            acc = acc + w[o, :cols][None, :] * d[:, o, None]
    assert acc.dtype == F
    return acc


def mask(dv, post_relu):
    """the ReLU's gradient: z > 0 passes (z == 0, z < 0 and NaN pass nothing)"""
    with np.errstate(invalid="ignore"):
        return np.where(post_relu > 0, dv, F(0)).astype(F)


def tile_gradients(sd, fw, td, B, r0, r1):
    rows = slice(r0, r1)
    with np.errstate(all="ignore"):
        e = (fw["q"][rows] - np.asarray(td, dtype=F)[rows]).astype(F)
        dq = (e * F(2.0 / B)).astype(F)
        sq = F(0)
        for r in range(e.shape[0]):
            sq = F(sq + F(e[r] * e[r]))
        g = {}
        g["fc_out.weight"], g["fc_out.bias"] = dw(dq[:, None], fw["h3"][rows])
        d3 = (dq[:, None] * np.asarray(sd["fc_out.weight"], dtype=F)[0][None, :]).astype(F)
        g["fc.weight"], g["fc.bias"] = dw(d3, fw["feat"][rows])
        d2 = mask(dx(d3, np.asarray(sd["fc.weight"], dtype=F), 64), fw["feat"][rows, :64])
        g["encoder.fc2.weight"], g["encoder.fc2.bias"] = dw(d2, fw["h1"][rows])
        d1 = mask(dx(d2, np.asarray(sd["encoder.fc2.weight"], dtype=F), 64), fw["h1"][rows])
        g["encoder.fc1.weight"], g["encoder.fc1.bias"] = dw(d1, fw["x0"][rows])
    return g, sq


def gradients(sd, x, actions, td, tile=TILE):
    """({key: gradient of mean((q - td)^2)}, the loss, q) of one critic: the tiles' partials added from +0.0, tiles ascending."""
    fw = forward(sd, x, actions)
    B = fw["q"].shape[0]
    total, sq = None, F(0)
    with np.errstate(all="ignore"):
        for r0 in range(0, B, tile):
            g, s = tile_gradients(sd, fw, td, B, r0, min(r0 + tile, B))
            total = {k: (np.zeros_like(v) + v).astype(F) for k, v in g.items()} if total is None else {k: (total[k] + v).astype(F) for k, v in g.items()}
            sq = F(F(sq) + s)
        loss = F(sq / F(B))
    return total, loss, fw["q"]


def adam_scalars(t, lr=3e-4, betas=(0.9, 0.999)):
    """(-step, s): step = lr / (1 - beta1^t), s = sqrt(1 - beta2^t) with the running products in double, each rounded to float32 once."""
    b1t, b2t = 1.0, 1.0
    for _ in range(int(t)):
        b1t, b2t = b1t * float(betas[0]), b2t * float(betas[1])
    return -F(float(lr) / (1.0 - b1t)), F(np.sqrt(1.0 - b2t))


def adam(p, g, m, v, t, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, scalars=None):
    """One step, t = the step's number from 1: m = m + (1 - b1)(g - m); v = v b2 + ((1 - b2) g) g; den = sqrt(v) / s + eps;
    p = p + ((-step) m) / den.  float32; 1 - beta is formed in double and rounded once."""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    nstep, s = scalars if scalars is not None else adam_scalars(t, lr, betas)
    b2, omb1, omb2 = F(betas[1]), F(1.0 - float(betas[0])), F(1.0 - float(betas[1]))
    with np.errstate(all="ignore"):
        m = (m + (omb1 * (g - m).astype(F)).astype(F)).astype(F)
        v = ((v * b2).astype(F) + ((omb2 * g).astype(F) * g).astype(F)).astype(F)
        den = ((np.sqrt(v).astype(F) / F(s)).astype(F) + F(eps)).astype(F)
        p = (p + ((F(nstep) * m).astype(F) / den).astype(F)).astype(F)
    return p, m, v
