"""DESIGN section 18's contract (tests/sac_critic_model.py) against the critic half of the reference's SACAgent.update, recorded by
tools/gen_sac_critic_goldens.py: no GPU needed.  Section 15's rule with its factor 4: the model may be as far from the float64 evaluation
as 4 times the reference's own float32 pipeline is.

Measured (model / reference, the worst network and update of a case; DESIGN section 18 has the table): gradients at most 1.76, q and loss
pooled 2.80, parameters behind Adam 1.00, exp_avg 1.88, exp_avg_sq 1.42."""
import glob
import json
import os

import numpy as np
import pytest

import sac_critic_model as cm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("o4_a1_s4", "o20_a4_s5", "o6_a2_s1", "o40_a8_s5")
UPDATES = {"o4_a1_s4": 3, "o20_a4_s5": 3, "o6_a2_s1": 3, "o40_a8_s5": 1}
F = np.float32
D = np.float64

_cases = {}


def load(case):
    """The case's inputs and, per (update, critic), the recorded step (its files merged)."""
    if case not in _cases:
        main = dict(np.load(os.path.join(GOLDEN, f"saccr_{case}.npz")))
        info = json.loads(str(main["info_json"]))
        steps = {}
        for u in range(info["updates"]):
            for c in (1, 2):
                files = sorted(glob.glob(os.path.join(GOLDEN, f"saccr_{case}_u{u}_c{c}*.npz")))
                assert files, (case, u, c)
                steps[(u, c)] = {k: v for f in files for k, v in np.load(f).items()}
        _cases[case] = (main, info, steps)
    return _cases[case]


def start(case, u, c):
    """(parameters, exp_avg, exp_avg_sq) of critic c before update u: the float32 chain of the reference."""
    main, info, steps = load(case)
    keys = info["keys"]
    if u == 0:
        p = {k: main[f"c{c}.{k}"] for k in keys}
        return p, {k: np.zeros_like(v) for k, v in p.items()}, {k: np.zeros_like(v) for k, v in p.items()}
    s = steps[(u - 1, c)]
    return tuple({k: s[f"{tag}32.{k}"] for k in keys} for tag in ("p", "m", "v"))


def ref64(s, tag, key):
    return s[f"{tag}32.{key}"].astype(D) - s[f"{tag}err.{key}"].astype(D)


def pooled(model, s, tag, keys):
    """(the model's error, the reference's) as max over the tensors of max|x - ref64| / max|ref64|"""
    mine, theirs = 0.0, 0.0
    for k in keys:
        want = ref64(s, tag, k)
        scale = np.max(np.abs(want))
        assert scale > 0 and model[k].dtype == F and model[k].shape == want.shape, (tag, k)
        mine = max(mine, float(np.max(np.abs(model[k].astype(D) - want)) / scale))
        theirs = max(theirs, float(np.max(np.abs(s[f"{tag}err.{k}"].astype(D))) / scale))
    return mine, theirs


def test_the_cases_are_the_issues():
    for case in CASES:
        main, info, steps = load(case)
        assert info["updates"] == UPDATES[case] and info["batch"] == 64 and main["states"].shape[:2] == (info["updates"], 64)
        assert len(steps) == 2 * info["updates"]
        assert (main["lr"], main["beta1"], main["beta2"], main["eps"]) == (3e-4, 0.9, 0.999, 1e-8)       # the reference's optimisers: torch's defaults
    for f in glob.glob(os.path.join(GOLDEN, "saccr_*.npz")):
        assert os.path.getsize(f) <= 666561, f


@pytest.mark.parametrize("case", CASES)
def test_gradients_loss_and_q_within_four_times_the_references_error(case):
    main, info, steps = load(case)
    keys = info["keys"]
    for u in range(info["updates"]):
        for c in (1, 2):
            p, _, _ = start(case, u, c)
            g, loss, q = cm.gradients(p, main["states"][u], main["actions"][u], main["td_target"][u])
            mine, theirs = pooled(g, steps[(u, c)], "g", keys)
            print(f"{case} update {u} critic {c}: gradients {mine:.3e} against {theirs:.3e} ({mine / theirs:.2f})")
            assert theirs > 0 and mine <= 4 * theirs, (u, c, mine, theirs)
            # q [B] and the loss [1] are the network's two forward tensors: the same pooled rule over them (the loss alone is ONE number,
            # whose float32 error in the reference is by luck 1 / 40 of an ulp in one of the recorded updates)
            q64, q32 = main["q64"][u, c - 1], main["q32"][u, c - 1]
            l64, l32 = main["loss64"][u, c - 1], main["loss32"][u, c - 1]
            assert q.dtype == F and type(loss) is F
            mq, tq = np.max(np.abs(q.astype(D) - q64)) / np.max(np.abs(q64)), np.max(np.abs(q32.astype(D) - q64)) / np.max(np.abs(q64))
            ml, tl = abs(D(loss) - l64) / abs(l64), abs(D(l32) - l64) / abs(l64)
            mine, theirs = max(mq, ml), max(tq, tl)
            print(f"    q {mq:.3e} against {tq:.3e}, loss {ml:.3e} against {tl:.3e}: pooled {mine / theirs:.2f}")
            assert theirs > 0 and mine <= 4 * theirs, (u, c, mq, tq, ml, tl)


@pytest.mark.parametrize("case", CASES)
def test_adam_within_four_times_the_references_error(case):
    main, info, steps = load(case)
    keys = info["keys"]
    hyper = dict(lr=float(main["lr"]), betas=(float(main["beta1"]), float(main["beta2"])), eps=float(main["eps"]))
    for u in range(info["updates"]):
        for c in (1, 2):
            p, m, v = start(case, u, c)
            s = steps[(u, c)]
            out = {"p": {}, "m": {}, "v": {}}
            for k in keys:
                out["p"][k], out["m"][k], out["v"][k] = cm.adam(p[k], s[f"g32.{k}"], m[k], v[k], u + 1, **hyper)
            for tag in ("p", "m", "v"):
                mine = max(float(np.max(np.abs(out[tag][k].astype(D) - ref64(s, tag, k)))) for k in keys)
                theirs = max(float(np.max(np.abs(s[f"{tag}err.{k}"].astype(D)))) for k in keys)
                print(f"{case} update {u} critic {c}: {tag} {mine:.3e} against {theirs:.3e} ({mine / theirs:.2f})")
                assert theirs > 0 and mine <= 4 * theirs, (u, c, tag, mine, theirs)


# ---------------------------------------------------------------------------------------------------- properties of the model itself
def small(rng, obs_w=3, act_w=2, S=2, B=37):
    from pednstream_amd.sac import critic_shapes

    sd = {k: (rng.uniform(-1, 1, size=shape) / np.sqrt(shape[-1] if len(shape) == 2 else 64) * 2).astype(F) for k, shape in critic_shapes(obs_w, act_w, S)}
    x = rng.standard_normal((B, S, obs_w)).astype(F)
    return sd, x, rng.standard_normal((B, act_w)).astype(F), rng.standard_normal(B).astype(F)


def test_the_relu_mask_passes_nothing_at_zero():
    """z == 0 exactly (a zero row of encoder.fc2 with a zero bias, and one with a bias that cancels): that neuron passes no gradient to
    what lies before it, as torch's threshold_backward (z > 0); -0.0 and NaN pass nothing either."""
    assert cm.mask(np.array([1, 2, 3, 4, 5], dtype=F), np.array([0.0, -0.0, np.nan, 1e-30, -1.0], dtype=F)).tolist() == [0, 0, 0, 4, 0]
    rng = np.random.default_rng(3)
    sd, x, a, td = small(rng)
    sd["encoder.fc2.weight"][5] = 0
    sd["encoder.fc2.bias"][5] = 0
    fw = cm.forward(sd, x, a)
    assert not fw["feat"][:, 5].any()
    g, _, _ = cm.gradients(sd, x, a, td)
    assert not g["encoder.fc2.weight"][5].any() and g["encoder.fc2.bias"][5] == 0 and np.abs(g["fc.weight"][:, 5]).max() == 0
    sd2 = {k: v.copy() for k, v in sd.items()}
    sd2["fc.weight"][:, 5] = 7.0                              # the gradient that arrives there is not zero; the mask stops it
    g2, _, _ = cm.gradients(sd2, x, a, td)
    assert not g2["encoder.fc2.weight"][5].any() and g2["encoder.fc2.bias"][5] == 0


def test_rows_beyond_the_batch_are_inert_and_tiles_are_the_order():
    rng = np.random.default_rng(4)
    sd, x, a, td = small(rng, B=70)
    g, loss, q = cm.gradients(sd, x[:37], a[:37], td[:37])
    # the rows behind the batch's last are never read: poison changes nothing
    x2, a2, td2 = x.copy(), a.copy(), td.copy()
    x2[37:], a2[37:], td2[37:] = np.nan, np.inf, np.nan
    g2, loss2, q2 = cm.gradients(sd, x2[:37], a2[:37], td2[:37])
    assert all(np.array_equal(g[k], g2[k]) for k in g) and loss == loss2 and np.array_equal(q, q2)
    # a non-finite row INSIDE the batch does reach its tile's sums
    x2[36] = np.nan
    g3, loss3, _ = cm.gradients(sd, x2[:37], a2[:37], td2[:37])
    assert np.isnan(loss3) and np.isnan(g3["fc_out.bias"]).all()
    # the tile is part of the order: another tile size gives close but not always equal bits; q does not depend on it
    g8, _, q8 = cm.gradients(sd, x[:37], a[:37], td[:37], tile=8)
    assert np.array_equal(q8, q) and any(not np.array_equal(g8[k], g[k]) for k in g)
    assert all(np.allclose(g8[k], g[k], rtol=1e-4, atol=1e-6) for k in g)
    # against float64 autograd-free algebra for the last layer: dL/d fc_out.bias = sum 2 (q - td) / B
    want = np.sum(2.0 * (q.astype(D) - td[:37].astype(D)) / 37)
    assert abs(g["fc_out.bias"][0] - want) <= 1e-5 * max(1.0, abs(want))


def test_gradients_change_nothing_but_their_outputs():
    """critic_gradients' semantics in the model: the parameters, the inputs and an optimiser state are read only, and a second
    evaluation gives the same bits."""
    rng = np.random.default_rng(5)
    sd, x, a, td = small(rng)
    keep = {k: v.copy() for k, v in sd.items()}, x.copy(), a.copy(), td.copy()
    g, loss, q = cm.gradients(sd, x, a, td)
    g2, loss2, q2 = cm.gradients(sd, x, a, td)
    assert all(np.array_equal(sd[k], keep[0][k]) for k in sd) and np.array_equal(x, keep[1]) and np.array_equal(a, keep[2]) and np.array_equal(td, keep[3])
    assert all(np.array_equal(g[k], g2[k]) and g[k].dtype == F and g[k].shape == sd[k].shape for k in sd) and loss == loss2 and np.array_equal(q, q2)
    m, v = np.full(4, 0.5, dtype=F), np.full(4, 0.25, dtype=F)
    p = np.ones(4, dtype=F)
    p2, m2, v2 = cm.adam(p, np.ones(4, dtype=F), m, v, 2)
    assert (p == 1).all() and (m == 0.5).all() and (v == 0.25).all() and not np.array_equal(p2, p) and not np.array_equal(m2, m)


def test_adam_leaves_zero_padding_and_matches_its_formulas():
    z = np.zeros(8, dtype=F)
    for t in (1, 2, 1000):
        p, m, v = cm.adam(z, z, z, z, t)
        assert not p.any() and not m.any() and not v.any() and not np.signbit(p).any()
    # the first step of a fresh state moves every parameter by lr against its gradient's sign (|g| >> eps)
    g = np.array([0.5, -2.0, 1e-3, -7e4], dtype=F)
    p, m, v = cm.adam(np.ones(4, dtype=F), g, np.zeros(4, dtype=F), np.zeros(4, dtype=F), 1, lr=1e-2)
    assert np.allclose(p, 1 - 1e-2 * np.sign(g), rtol=0, atol=1e-6)
    assert np.allclose(m, 0.1 * g, rtol=1e-6) and np.allclose(v, 1e-3 * g.astype(D) ** 2, rtol=1e-5)
    nstep, s = cm.adam_scalars(3)
    assert nstep == -F(3e-4 / (1 - 0.9 ** 3)) or abs(float(nstep) + 3e-4 / (1 - 0.9 ** 3)) < 1e-10
    assert abs(float(s) - np.sqrt(1 - 0.999 ** 3)) < 1e-8
