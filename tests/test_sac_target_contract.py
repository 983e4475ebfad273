"""The numpy model of the SAC TD targets and the Polyak update (tests/sac_target_model.py) against what the reference's
own SACAgent computed (tests/golden/sactd_*.npz, written by tools/gen_sac_target_goldens.py), and hand-built checks of the contract's
corners.  No GPU."""
import glob
import json
import os
import sys

import numpy as np
import pytest

import actor_model as am
import sac_target_model as sm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rng_contract  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(4, 1, 4), (20, 4, 5), (56, 8, 5), (6, 2, 1)]
LOG_ALPHAS = [np.log(0.01), 0.3, -1.0, np.log(0.01)]
B = 256
MARGIN = 4.0        # the model may be this many times as far from the float64 results as the reference's own float32 pipeline is
OUTPUTS = ("mu", "std", "logp", "next_actions", "entropy", "q1", "q2", "td_target")
F = np.float32
_cache = {}


def sds(z, tags):
    return [{k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + ".")} for tag in tags]


def load(o, a, s):
    key = (o, a, s)
    if key not in _cache:
        z = np.load(os.path.join(GOLDEN, f"sactd_o{o}_a{a}_s{s}.npz"))
        actor, tc1, tc2 = sds(z, ("actor", "tc1", "tc2"))
        out = sm.target(actor, tc1, tc2, z["x"], z["rewards"], z["dones"], z["eps"], z["log_alpha"], float(z["gamma"]), float(z["max_delta"]))
        _cache[key] = (z, actor, tc1, tc2, out)
    return _cache[key]


def test_every_case_has_its_fixture():
    assert len(glob.glob(os.path.join(GOLDEN, "sactd_o*.npz"))) == len(CASES)
    assert len(glob.glob(os.path.join(GOLDEN, "sactd_polyak_o*.npz"))) == len(CASES)
    for (o, a, s), la in zip(CASES, LOG_ALPHAS):
        z, actor, tc1, tc2, _ = load(o, a, s)
        info = json.loads(str(z["info_json"]))
        assert (info["obs_dim"], info["act_dim"], info["stack_size"]) == (o, a, s)
        assert z["x"].shape == (B, s, o) and z["x"].dtype == np.float32
        assert z["rewards"].shape == (B,) and z["dones"].shape == (B,) and z["eps"].shape == (B, a) and z["eps"].dtype == np.float32
        assert 0 < z["dones"].sum() < B and set(np.unique(z["dones"])) == {0.0, 1.0}
        assert z["log_alpha"] == np.float32(la) and float(z["gamma"]) == 0.99 and float(z["tau"]) == 0.005
        assert actor["fc_std.weight"].shape == (a, 64)
        for c in (tc1, tc2):
            assert c["encoder.fc1.weight"].shape == (64, o * s) and c["fc.weight"].shape == (64, 64 + a + 1) and c["fc_out.weight"].shape == (1, 64)
        for name in OUTPUTS:
            want = (B, a) if name in ("mu", "std", "logp", "next_actions") else (B,)
            assert z[name + "32"].shape == want and z[name + "32"].dtype == np.float32, name
            assert z[name + "64"].shape == want and z[name + "64"].dtype == np.float64, name
        assert 0.05 <= z["std32"].min() and z["std32"].max() <= 20.0
        lower = z["q232"] < z["q132"]
        assert lower.any() and not lower.all()                       # the minimum switches between the critics
        with np.load(os.path.join(GOLDEN, f"sactd_polyak_o{o}_a{a}_s{s}.npz")) as p:
            for tag in ("c1", "c2", "after1", "after2"):
                assert {k[len(tag) + 1:] for k in p.files if k.startswith(tag + ".")} == set(tc1), tag


@pytest.mark.parametrize("o,a,s", CASES)
def test_model_is_as_close_to_float64_as_the_reference(o, a, s):
    z, actor, tc1, tc2, out = load(o, a, s)
    for name in OUTPUTS:
        e_ref = np.max(np.abs(z[name + "32"].astype(np.float64) - z[name + "64"]))
        e_model = np.max(np.abs(out[name].astype(np.float64) - z[name + "64"]))
        print(f"({o}, {a}, {s}) {name}: model {e_model:.3e}  reference {e_ref:.3e}  ratio {e_model / e_ref:.2f}")
        assert e_ref > 0, name
        assert e_model <= MARGIN * e_ref, (name, e_model, e_ref)


@pytest.mark.parametrize("o,a,s", CASES)
def test_polyak_model_equals_the_reference_bit_for_bit(o, a, s):
    z, actor, tc1, tc2, _ = load(o, a, s)
    p = np.load(os.path.join(GOLDEN, f"sactd_polyak_o{o}_a{a}_s{s}.npz"))
    c1, c2, after1, after2 = sds(p, ("c1", "c2", "after1", "after2"))
    tau = float(z["tau"])
    for before, online, after in ((tc1, c1, after1), (tc2, c2, after2)):
        for k in before:
            got = sm.polyak(before[k], online[k], tau)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), after[k].view(np.uint32)), k
            assert not np.array_equal(after[k], before[k])


# ---------------------------------------------------------------------------------------------------- hand-built checks
def zero_critic(obs_w, act_w, S):
    return {"encoder.fc1.weight": np.zeros((64, S * obs_w), F), "encoder.fc1.bias": np.zeros(64, F), "encoder.fc2.weight": np.zeros((64, 64), F),
            "encoder.fc2.bias": np.zeros(64, F), "fc.weight": np.zeros((64, 64 + act_w + 1), F), "fc.bias": np.zeros(64, F),
            "fc_out.weight": np.zeros((1, 64), F), "fc_out.bias": np.zeros(1, F)}


def test_feature_order_and_the_gate_width_column():
    """feat = [encoder (64), next_action (act_w), x[b, S - 1, obs_w - 1]]: an identity-like fc hands feature i to neuron i, and fc_out picks it."""
    S, obs_w, act_w = 3, 5, 2
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4, S, obs_w)).astype(F)
    na = rng.standard_normal((4, act_w)).astype(F)
    sd = zero_critic(obs_w, act_w, S)
    sd["encoder.fc2.bias"][:] = np.arange(64, dtype=F) + 1                     # the encoder's outputs: 1 .. 64 (ReLU keeps them)
    for i in range(64):
        sd["fc.weight"][i, i] = 1
    sd["fc.weight"][0, 64], sd["fc.weight"][1, 65], sd["fc.weight"][2, 66] = 1, 1, 1      # neurons 0, 1, 2 also see next_action and g
    h_want = np.tile(np.arange(64, dtype=F) + 1, (4, 1))
    h_want[:, 0] += na[:, 0]
    h_want[:, 1] += na[:, 1]
    h_want[:, 2] += x[:, S - 1, obs_w - 1]
    for i in (0, 1, 2, 7, 63):
        sd["fc_out.weight"][:] = 0
        sd["fc_out.weight"][0, i] = 1
        assert np.array_equal(sm.critic(sd, x, na), h_want[:, i]), i
    # the column is the NEWEST frame's LAST one, no other
    y = x.copy()
    y[:, :S - 1, :] += 1
    y[:, S - 1, :obs_w - 1] += 1
    sd["fc_out.weight"][:] = 0
    sd["fc_out.weight"][0, 2] = 1
    assert np.array_equal(sm.critic(sd, y, na), h_want[:, 2])


def test_no_relu_between_fc_and_fc_out():
    S, obs_w, act_w = 1, 2, 1
    sd = zero_critic(obs_w, act_w, S)
    sd["fc.bias"][:] = -2                                                      # a ReLU would turn every neuron into 0
    sd["fc_out.weight"][0, :] = 1
    q = sm.critic(sd, np.zeros((1, S, obs_w), F), np.zeros((1, act_w), F))
    assert q[0] == -128.0
    # the encoder has its two
    sd["encoder.fc1.bias"][:] = -1
    sd["encoder.fc2.weight"][:] = 1
    sd["fc.weight"][0, 0] = 1
    assert sm.critic(sd, np.zeros((1, S, obs_w), F), np.zeros((1, act_w), F))[0] == -128.0


def test_done_drops_the_bootstrap_and_nan_reaches_the_target():
    q1, q2 = np.array([1, 5, np.nan, 2], F), np.array([3, 4, 1, np.nan], F)
    assert np.array_equal(sm.q_min(q1, q2)[:2], np.array([1, 4], F)) and np.isnan(sm.q_min(q1, q2)[2:]).all()
    ent, r = np.array([2, 2, 2, 2], F), np.array([10, 20, 30, 40], F)
    t = sm.td(q1, q2, ent, np.log(0.5), r, np.array([0, 1, 0, 0], F), gamma=0.5)
    alpha = F(np.exp(np.float64(F(np.log(0.5)))))
    assert t[0] == F(10) + F(0.5) * (F(1) + alpha * F(2)) and t[1] == 20 and np.isnan(t[2]) and np.isnan(t[3])
    # ... and done = 1 does not hide a NaN critic (NaN * 0 is NaN, as in torch)
    assert np.isnan(sm.td(q1, q2, ent, np.log(0.5), r, np.ones(4, F))[2])
    # entropy: ((0 - l0) - l1) - l2, one rounding each
    lp = np.array([[2.0 ** 24, 1, -2.0 ** 24]], F)
    assert sm.entropy(lp)[0] == F(F(F(0) - lp[0, 0]) - lp[0, 1]) - lp[0, 2] == 0.0


def test_log_probability_mirrors_the_second_tanh():
    mu, std, eps = np.array([[0.3]], F), np.array([[0.7]], F), np.array([[1.1]], F)
    u, t, na, logp = sm.tail(mu, std, eps, 2.5)
    U = np.float64(u[0, 0])
    want = -((U - 0.3) ** 2) / (2 * 0.7 ** 2) - np.log(0.7) - 0.5 * np.log(2 * np.pi) - np.log(1 - np.tanh(np.tanh(U)) ** 2 + 1e-7)
    assert abs(logp[0, 0] - want) < 1e-6
    once = -((U - 0.3) ** 2) / (2 * 0.7 ** 2) - np.log(0.7) - 0.5 * np.log(2 * np.pi) - np.log(1 - np.tanh(U) ** 2 + 1e-7)
    assert abs(logp[0, 0] - once) > 1e-2
    assert na[0, 0] == F(t[0, 0] * F(2.5)) and t[0, 0] == F(np.tanh(U))


def test_noise_stream_is_its_own():
    for b, c, d, seed in ((0, 0, 0, 7), (4095, 7, 3, 7), (17, 2, 2 ** 32 + 5, 0x1234567890)):
        w = rng_contract.philox4x32_10((b, d & 0xFFFFFFFF, 0x73 | (c << 8), d >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        u1, u2 = (w[0] + 1) * 2.0 ** -32, w[1] * 2.0 ** -32
        assert sm.noise(seed, b, c, d) == np.float32(np.sqrt(-2 * np.log(u1)) * np.cos(6.283185307179586 * u2))
    b, c = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
    mine, actors = sm.noise(7, b, c, 0), am.noise(7, b, c, 0)
    assert sm.NOISE_SITE == 0x73 and am.NOISE_SITE == 0x72
    assert not np.any(mine.view(np.uint32) == actors.view(np.uint32))
    assert not np.any(sm.noise(7, b, c, 1).view(np.uint32) == mine.view(np.uint32))


def test_polyak_model_is_torchs_two_multiplies_and_an_add():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    t, o = rng.standard_normal(100000).astype(F), rng.standard_normal(100000).astype(F)
    for tau in (0.005, 0.3, 1e-3, 0.0, 1.0):
        want = (torch.tensor(t) * (1.0 - tau) + torch.tensor(o) * tau).numpy()
        assert np.array_equal(sm.polyak(t, o, tau).view(np.uint32), want.view(np.uint32)), tau
