"""Edge cases of the recurrent PPO agents' clipped-loss epochs ("Edges"): TEST INFRASTRUCTURE, importable without a
device.  tests/test_lstm_update_edges_host.py proves on the CPU that these inputs reach the edges they are named for;
tests/test_gpu_lstm_update_edges.py runs them through the kernels.

    doctor(sd)                      -> a copy of a recurrent network's state dict (actor or value) whose units 0-9 sit on the ends of the cell
    edge_conditions(fw)             -> {name: bool}: what a forward (lstm_update_model.forward's dict) of a doctored network exhibits
    WIDE_AGENTS                     -> a second agent table: obs_w that fill one and two chunks of 32 inputs and one over two, act_w 5, 7, 8
    shifted / on_clip_bounds / beyond_twenty(logp, ...) -> old_log_probs that put the ratios around 1, on 1 +- clip_eps, beyond exp(+-20)
    flush_subnormals, mask_passing_zero, tail_without_ps, tail_without_pl -> the WRONG variants of the model's pieces the host test patches in
"""
import numpy as np

F = np.float32
H = 64
TINY = np.finfo(F).tiny                          # 2^-126: below it a non-zero float32 is subnormal
GATES = {"i": 0, "f": 1, "g": 2, "o": 3}         # row gate * 64 + unit
# (unit, gate, bias_ih): bias_hh of the row is 0, the row's weights stay.  sigmoid(-200) and sigmoid(-600) round to 0.0f, the latter through
# exp's branch for 512 <= |x| < 1024, sigmoid(-2000) through the one beyond 1024; sigmoid(-95) is a float32 subnormal; tanh(300) reads
# exp(-600), tanh(-2000) exp(-4000).
BIASES = ((1, "o", -200.0), (2, "i", 200.0), (2, "f", -200.0), (3, "f", -95.0), (4, "o", -95.0), (5, "g", 300.0), (6, "i", 600.0),
          (7, "f", -2000.0), (8, "o", -600.0), (9, "g", -2000.0))

# (obs0, obs_w, act0, act_w).  Observation columns 0, 33-34, 99 and 165-166 and action columns 0, 13 and 22 belong to nobody.
WIDE_AGENTS = [(1, 32, 1, 5), (35, 64, 6, 7), (100, 65, 14, 8)]
WIDE_N_OBS, WIDE_N_ACTIONS = 167, 23


def doctor(sd):
    """Unit 0: all four gate rows of weight_ih and weight_hh and both biases zero (i = f = o = 0.5, g = 0, so c' = h' = +0.0 at every
    step).  Units 1-9: BIASES."""
    out = {k: np.array(v, dtype=F) for k, v in sd.items()}
    for g in range(4):
        for key in ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"):
            out[key][g * H] = 0
    for unit, gate, bias in BIASES:
        row = GATES[gate] * H + unit
        out["lstm.bias_ih_l0"][row], out["lstm.bias_hh_l0"][row] = F(bias), F(0)
    return out


_doctored = {}


def doctored(c):
    """(actors, values): the doctored state dicts of a setup's networks (c["actors"], c["values"]), made once per setup"""
    if id(c) not in _doctored:
        _doctored[id(c)] = (c, [doctor(sd) for sd in c["actors"]], [doctor(sd) for sd in c["values"]])
    return _doctored[id(c)][1:]


def subnormal(v):
    v = np.abs(np.asarray(v, dtype=F))
    return (v > 0) & (v < TINY)


def edge_conditions(fw):
    h, i, f, g, o = (np.asarray(fw[k], dtype=F) for k in "hifgo")
    zero = h == 0
    return {
        "unit 0: h' is +0.0 at every step": bool((zero[:, :, 0] & ~np.signbit(h[:, :, 0])).all()),
        "unit 1: o == 0.0": bool((o[:, :, 1] == 0).all()),
        "h' holds +0.0 and -0.0": bool((zero & np.signbit(h)).any() and (zero & ~np.signbit(h)).any()),
        "unit 2: i == 1.0 and f == 0.0": bool((i[:, :, 2] == 1).all() and (f[:, :, 2] == 0).all()),
        "unit 3: a subnormal f": bool(subnormal(f[:, :, 3]).any()),
        "unit 4: a subnormal o and a subnormal h'": bool(subnormal(o[:, :, 4]).any() and subnormal(h[:, :, 4]).any()),
        "unit 5: g == 1.0": bool((g[:, :, 5] == 1).all()),
        "unit 6: i == 1.0": bool((i[:, :, 6] == 1).all()),
        "unit 7: f == 0.0": bool((f[:, :, 7] == 0).all()),
        "unit 8: o == 0.0": bool((o[:, :, 8] == 0).all()),
        "unit 9: g == -1.0": bool((g[:, :, 9] == -1).all()),
    }


# ---------------------------------------------------------------------------------------------------- old_log_probs of the tail's corners
def shifted(logp, shift):
    """ratios around 1 +- 0.25, as tests/test_gpu_lstm_update.py's"""
    return (np.asarray(logp, dtype=F) + np.asarray(shift, dtype=F)).astype(F)


def on_clip_bounds(logp, clip_eps=0.2):
    """step 0: old = logp - log(F(1 + clip_eps)), step 1: old = logp - log(F(1 - clip_eps)): some ratios land exactly on a bound"""
    old = np.array(logp, dtype=F)
    old[0] = old[0] - F(np.log(np.float64(F(1.0 + clip_eps))))
    old[1] = old[1] - F(np.log(np.float64(F(1.0 - clip_eps))))
    return old


def beyond_twenty(logp):
    """step 0: logp - old = +25, step 1: -25 (in float32 within an ulp of it, far from 20): the clamp of the log-ratio blocks d logp"""
    old = np.array(logp, dtype=F)
    old[0] = old[0] - F(25)
    old[1] = old[1] + F(25)
    return old


# ---------------------------------------------------------------------------------------------------- wrong variants of the model's pieces
def flush_subnormals(fn):
    """fn (lstm_model.sigmoid) with subnormal results flushed to +0.0, as a kernel built to flush them would give"""
    def flushed(z):
        y = fn(z)
        return np.where(subnormal(y), F(0), y).astype(F)
    return flushed


def mask_passing_zero(dv, post_relu):
    """sac_critic_model.mask with >= in place of >"""
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(post_relu) >= 0, dv, F(0)).astype(F)


def tail_without_ps(tail):
    """ppo_update_model.tail whose std clamp passes its gradient everywhere (min_std, max_std are read by ps alone)"""
    def variant(fw, old, adv, R, clip_eps=0.2, min_std=1e-3, max_std=10.0):
        return tail(fw, old, adv, R, clip_eps, -np.inf, np.inf)
    return variant


def tail_without_pl(tail):
    """ppo_update_model.tail whose +-20 clamp of the log-ratio passes its gradient: where |logp - old| > 20 it is handed logp = +-20 and
    old = 0, a log-ratio exactly ON the clamp, which gives the same ratio and pl = 1 (d_mu and d_z read logp and old through their
    difference only)"""
    def variant(fw, old, adv, R, clip_eps=0.2, min_std=1e-3, max_std=10.0):
        lp, old = np.asarray(fw["logp"], dtype=F), np.asarray(old, dtype=F)
        with np.errstate(all="ignore"):
            dl = (lp - old).astype(F)
        far = np.abs(dl) > F(20)
        fw = dict(fw, logp=np.where(far, np.clip(dl, F(-20), F(20)), lp).astype(F))
        return tail(fw, np.where(far, F(0), old).astype(F), adv, R, clip_eps, min_std, max_std)
    return variant
