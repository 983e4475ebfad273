"""DESIGN section 19's contract (tests/sac_actor_model.py) against the actor half of the reference's SACAgent.update, recorded by
tools/gen_sac_actor_goldens.py: no GPU needed.  Sections 15 and 18's rule with the project's factor 4: the model may be as far from the
float64 evaluation as 4 times the reference's own float32 pipeline is.

Measured (model / reference, the worst update of a case; DESIGN section 19 has the table): gradients at most 0.93, the forward's tensors
and scalars pooled 2.10, parameters behind Adam 1.00, exp_avg 1.30, exp_avg_sq 1.00.  With section 18's exp_avg_sq, every product rounded,
the last was 4.83 in case (6, 2, 1), update 1 (1.835e-11 against 3.799e-12: fc_mu.bias[1] = 1.4e-4 lay 1.26 ulp from the float64 step, the
reference 0.26): the step fuses that multiply-add now, as torch's does."""
import glob
import json
import os

import numpy as np
import pytest

import sac_actor_model as mm
import sac_critic_model as cm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("o4_a1_s4", "o20_a4_s5", "o6_a2_s1", "o40_a8_s5")
UPDATES = {"o4_a1_s4": 3, "o20_a4_s5": 3, "o6_a2_s1": 3, "o40_a8_s5": 1}
FORWARD = ("mu", "std", "logp", "entropy", "q1", "q2", "actor_loss", "alpha_loss", "alpha_grad")
CRITIC_KEYS = [f"{layer}.{part}" for layer in ("encoder.fc1", "encoder.fc2", "fc", "fc_out") for part in ("weight", "bias")]
F = np.float32
D = np.float64

_cases = {}


def load(case):
    """The case's inputs and, per update, the recorded step (its files merged)."""
    if case not in _cases:
        main = dict(np.load(os.path.join(GOLDEN, f"sacac_{case}.npz")))
        info = json.loads(str(main["info_json"]))
        steps = {}
        for u in range(info["updates"]):
            files = sorted(glob.glob(os.path.join(GOLDEN, f"sacac_{case}_u{u}*.npz")))
            assert files, (case, u)
            steps[u] = {k: v for f in files for k, v in np.load(f).items()}
        _cases[case] = (main, info, steps)
    return _cases[case]


def start(case, u):
    """(parameters, exp_avg, exp_avg_sq) of the actor and of log_alpha (key "log_alpha") before update u: the reference's float32 chain."""
    main, info, steps = load(case)
    keys = info["keys"]
    if u == 0:
        p = {k: main[f"actor.{k}"] for k in keys}
        p["log_alpha"] = main["log_alpha"][0]
        return p, {k: np.zeros_like(v) for k, v in p.items()}, {k: np.zeros_like(v) for k, v in p.items()}
    s = steps[u - 1]
    return tuple({k: s[f"{tag}32.{k}"] for k in keys + ["log_alpha"]} for tag in ("p", "m", "v"))


def model(case, u):
    main, info, steps = load(case)
    p, _, _ = start(case, u)
    assert p["log_alpha"] == main["log_alpha"][u]
    c1, c2 = ({k: steps[u][f"c{c}.{k}"] for k in CRITIC_KEYS} for c in (1, 2))
    return mm.gradients(p, c1, c2, main["states"][u], main["eps"][u], p["log_alpha"], main["target_entropy"], float(main["max_delta"]))


def test_the_cases_are_the_issues():
    for case in CASES:
        main, info, steps = load(case)
        assert info["updates"] == UPDATES[case] and info["batch"] == 64 and main["states"].shape[:2] == (info["updates"], 64)
        assert (main["lr"], main["alpha_lr"], main["beta1"], main["beta2"], main["eps_adam"]) == (3e-4, 3e-4, 0.9, 0.999, 1e-8)      # the reference's defaults
        assert main["target_entropy"] == -info["act_dim"]
        # what the tool asserted when it recorded: both critics selected in every update, section 15's guard on std, and a margin between
        # q1 and q2 far above q's float32 error, so that no row's gradient differs by a whole critic
        assert all(0 < n < 64 for n in info["q2_lower_rows"]) and 0.05 <= info["std_min"] and info["std_max"] <= 20
        q_error = max(np.abs(main[f"{q}err"]).max() for q in ("q1", "q2"))
        assert info["smallest_q_margin"] > 100 * q_error
        assert np.array_equal(main["q232"] < main["q132"], (main["q232"].astype(D) - main["q2err"]) < (main["q132"].astype(D) - main["q1err"]))
    for f in glob.glob(os.path.join(GOLDEN, "sacac_*.npz")):
        assert os.path.getsize(f) <= 666561, f


@pytest.mark.parametrize("case", CASES)
def test_gradients_and_forward_within_four_times_the_references_error(case):
    main, info, steps = load(case)
    keys = info["keys"]
    assert len(keys) == 10
    for u in range(info["updates"]):
        g, sc, fw = model(case, u)
        s = steps[u]
        mine, theirs = 0.0, 0.0
        for k in keys:
            want = s[f"g32.{k}"].astype(D) - s[f"gerr.{k}"].astype(D)
            scale = np.max(np.abs(want))
            assert scale > 0 and g[k].dtype == F and g[k].shape == want.shape, k
            mine = max(mine, float(np.max(np.abs(g[k].astype(D) - want)) / scale))
            theirs = max(theirs, float(np.max(np.abs(s[f"gerr.{k}"].astype(D))) / scale))
        print(f"{case} update {u}: gradients {mine:.3e} against {theirs:.3e} ({mine / theirs:.2f})")
        assert theirs > 0 and mine <= 4 * theirs, (u, mine, theirs)
        # the forward's tensors and the three scalars: the same pooled rule
        mine, theirs = 0.0, 0.0
        got = dict(fw, **sc)
        for name in FORWARD:
            r32, rerr = main[name + "32"][u], main[name + "err"][u].astype(D)
            want = r32.astype(D) - rerr
            scale = np.max(np.abs(want))
            x = np.asarray(got[name])
            assert scale > 0 and x.dtype == F and x.shape == want.shape, name
            mine = max(mine, float(np.max(np.abs(x.astype(D) - want)) / scale))
            theirs = max(theirs, float(np.max(np.abs(rerr)) / scale))
        print(f"    forward {mine:.3e} against {theirs:.3e} ({mine / theirs:.2f})")
        assert theirs > 0 and mine <= 4 * theirs, (u, "forward", mine, theirs)


@pytest.mark.parametrize("case", CASES)
def test_adam_within_four_times_the_references_error(case):
    main, info, steps = load(case)
    keys = info["keys"]
    kw = dict(betas=(float(main["beta1"]), float(main["beta2"])), eps=float(main["eps_adam"]))
    for u in range(info["updates"]):
        p, m, v = start(case, u)
        s = steps[u]
        out = {"p": {}, "m": {}, "v": {}}
        for k in keys:
            out["p"][k], out["m"][k], out["v"][k] = mm.adam(p[k], s[f"g32.{k}"], m[k], v[k], u + 1, lr=float(main["lr"]), **kw)
        k = "log_alpha"
        out["p"][k], out["m"][k], out["v"][k] = mm.adam(p[k], main["alpha_grad32"][u], m[k], v[k], u + 1, lr=float(main["alpha_lr"]), **kw)
        # one maximum over the actor's ten tensors and log_alpha beside them: log_alpha's moments and value are ONE number each, whose
        # float32 error in the reference is by luck anything down to nothing (section 18 pooled its loss with q for the same reason)
        names = keys + ["log_alpha"]
        for tag in ("p", "m", "v"):
            ref64 = lambda k: s[f"{tag}32.{k}"].astype(D) - s[f"{tag}err.{k}"].astype(D)
            mine = max(float(np.max(np.abs(out[tag][k].astype(D) - ref64(k)))) for k in names)
            theirs = max(float(np.max(np.abs(s[f"{tag}err.{k}"].astype(D)))) for k in names)
            print(f"{case} update {u}: {tag} {mine:.3e} against {theirs:.3e} ({mine / theirs:.2f})")
            assert theirs > 0 and mine <= 4 * theirs, (u, tag, mine, theirs)


# ---------------------------------------------------------------------------------------------------- properties of the model itself
def small(rng, obs_w=3, act_w=2, S=2, B=37):
    from pednstream_amd.policy import tensor_shapes
    from pednstream_amd.sac import critic_shapes

    draw = lambda shapes: {k: (rng.uniform(-1, 1, size=shape) / np.sqrt(shape[-1] if len(shape) == 2 else 64) * 2).astype(F) for k, shape in shapes}
    actor, c1, c2 = draw(tensor_shapes("sac", obs_w, act_w, S)), draw(critic_shapes(obs_w, act_w, S)), draw(critic_shapes(obs_w, act_w, S))
    return actor, c1, c2, rng.standard_normal((B, S, obs_w)).astype(F), rng.standard_normal((B, act_w)).astype(F)


def test_the_relu_masks_pass_nothing_at_zero():
    """h == 0 exactly, -0.0 and NaN behind a ReLU pass no gradient to what lies before it, as torch's threshold_backward (h > 0)."""
    with np.errstate(invalid="ignore"):
        assert cm.mask(np.ones(4, dtype=F), np.array([0.0, -0.0, np.nan, 1e-30], dtype=F)).tolist() == [0.0, 0.0, 0.0, 1.0]
    actor, c1, c2, x, eps = small(np.random.default_rng(1))
    actor["fc.weight"][5], actor["fc.bias"][5] = 0.0, 0.0              # h3[:, 5] == 0 in every row
    actor["encoder.fc2.weight"][7], actor["encoder.fc2.bias"][7] = 0.0, -0.0
    g, _, fw = mm.gradients(actor, c1, c2, x, eps, -1.0, -2.0)
    assert not fw["h3"][:, 5].any() and not fw["h2"][:, 7].any()
    assert not g["fc.weight"][5].any() and g["fc.bias"][5] == 0 and not g["encoder.fc2.weight"][7].any()
    assert g["fc_mu.weight"].any() and g["encoder.fc1.weight"].any() and not g["fc_mu.weight"][:, 5].any()


def test_a_tie_splits_in_halves_as_torch_does():
    torch = pytest.importorskip("torch")
    q1 = torch.tensor([1.0, 2.0, 3.0, float("nan")], requires_grad=True)
    q2 = torch.tensor([1.0, 3.0, 2.0, 0.5], requires_grad=True)
    torch.min(q1, q2).sum().backward()
    w1, w2 = mm.min_weights(q1.detach().numpy(), q2.detach().numpy())
    assert w1.tolist() == q1.grad.tolist() == [0.5, 1.0, 0.0, 1.0] and w2.tolist() == q2.grad.tolist() == [0.5, 0.0, 1.0, 1.0]
    # two equal critics: every row is a tie, and the gradient is that of either critic alone
    actor, c1, c2, x, eps = small(np.random.default_rng(2))
    tie, _, fw = mm.gradients(actor, c1, c1, x, eps, -1.0, -2.0)
    assert np.array_equal(fw["q1"], fw["q2"])
    d_tie = mm.head_gradients(fw, mm.dq_daction(c1, 2), mm.dq_daction(c1, 2), -1.0, 37)
    fw["q2"] = fw["q1"] + F(1)
    d_one = mm.head_gradients(fw, mm.dq_daction(c1, 2), mm.dq_daction(c2, 2), -1.0, 37)
    assert all(np.array_equal(a, b) for a, b in zip(d_tie, d_one))


def test_softplus_takes_its_linear_branch_above_20():
    actor, c1, c2, x, eps = small(np.random.default_rng(3), B=4)
    fw = mm.forward(actor, c1, c2, x, eps * F(0.01))
    v1, v2 = mm.dq_daction(c1, 2), mm.dq_daction(c2, 2)
    for z, factor in ((F(20.0), 1.0 / (1.0 + np.exp(-20.0))), (np.nextafter(F(20.0), F(30.0)), 1.0), (F(25.0), 1.0)):
        hi = dict(fw, z=np.full_like(fw["z"], z), std=np.full_like(fw["std"], z))      # (softplus(z) == z to float32 from 17 on)
        d_mu, d_z = mm.head_gradients(hi, v1, v2, -1.0, 4)
        alpha, G = D(mm.alpha_of(-1.0)), 0.25
        gsd = d_mu.astype(D) * hi["eps"].astype(D) - alpha * G / D(z)
        assert np.allclose(d_z, gsd * factor, rtol=1e-6, atol=0), z
    assert mm.am.softplus(np.array([25.0], dtype=F))[0] == F(25.0)


def test_rows_beyond_the_batch_are_inert_and_tiles_are_the_order():
    actor, c1, c2, x, eps = small(np.random.default_rng(4), B=70)
    g, sc, fw = mm.gradients(actor, c1, c2, x, eps, -1.0, -2.0)
    # the tiles' partials, added from +0.0 with tiles ascending, are the gradient; another tile is another order of the same sum
    parts = [mm.tile_gradients(actor, fw, fw["d_mu"], fw["d_z"], r0, min(r0 + 32, 70)) for r0 in (0, 32, 64)]
    for k in g:
        total = np.zeros_like(g[k])
        for part in parts:
            total = (total + part[k]).astype(F)
        assert np.array_equal(total, g[k]), k
    other, sc7, _ = mm.gradients(actor, c1, c2, x, eps, -1.0, -2.0, tile=7)
    assert any(not np.array_equal(other[k], g[k]) for k in g) and all(np.allclose(other[k], g[k], rtol=1e-3, atol=1e-6) for k in g)
    # rows behind the batch take no part: a tile's partial of rows [64, 70) does not depend on what lies behind row 70
    big = np.concatenate([x, np.full((5,) + x.shape[1:], np.nan, dtype=F)])
    fwb = mm.forward(actor, c1, c2, big, np.concatenate([eps, np.full((5, eps.shape[1]), np.inf, dtype=F)]))
    dmu, dz = (np.concatenate([d, np.full((5, d.shape[1]), np.nan, dtype=F)]) for d in (fw["d_mu"], fw["d_z"]))
    tail = mm.tile_gradients(actor, fwb, dmu, dz, 64, 70)
    assert all(np.array_equal(tail[k], parts[2][k]) for k in tail)


def test_gradients_change_nothing_and_the_critics_are_never_written():
    actor, c1, c2, x, eps = small(np.random.default_rng(5))
    keep = [{k: v.copy() for k, v in sd.items()} for sd in (actor, c1, c2)]
    g, sc, _ = mm.gradients(actor, c1, c2, x, eps, -1.0, -2.0)
    p, m, v = mm.adam(actor["fc.weight"], g["fc.weight"], np.zeros_like(g["fc.weight"]), np.zeros_like(g["fc.weight"]), 1)
    for sd, was in zip((actor, c1, c2), keep):
        assert all(np.array_equal(sd[k], was[k]) for k in sd)
    assert not np.array_equal(p, actor["fc.weight"]) and type(sc["actor_loss"]) is F and sc["alpha_loss"] == sc["alpha_grad"]
