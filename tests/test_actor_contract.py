"""The numpy model of the stacked actors (tests/actor_model.py) against what the reference's own modules computed
(tests/golden/actor_*.npz, written by tools/gen_actor_goldens.py), and the noise contract on the model.  No GPU."""
import glob
import json
import os
import sys

import numpy as np
import pytest

import actor_model as am

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rng_contract  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(kind, o, a, s) for (o, a, s) in ((4, 1, 4), (20, 4, 5), (56, 8, 5), (6, 2, 1)) for kind in ("sac", "ppo")]
MARGIN = 4.0        # the model may be this many times as far from the float64 forward as the reference's own float32 forward is
_cache = {}


def load(kind, o, a, s):
    key = (kind, o, a, s)
    if key not in _cache:
        z = np.load(os.path.join(GOLDEN, f"actor_{kind}_o{o}_a{a}_s{s}.npz"))
        sd = {k[3:]: z[k] for k in z.files if k.startswith("sd.")}
        mu, pre, std = am.forward(kind, sd, z["x"])
        _cache[key] = (z, sd, mu, pre, std)
    return _cache[key]


def test_every_case_has_its_fixture():
    assert len(glob.glob(os.path.join(GOLDEN, "actor_*.npz"))) == len(CASES)
    for kind, o, a, s in CASES:
        z, sd, *_ = load(kind, o, a, s)
        info = json.loads(str(z["info_json"]))
        assert (info["kind"], info["obs_dim"], info["act_dim"], info["stack_size"]) == (kind, o, a, s)
        assert z["x"].shape == (64, s, o) and z["x"].dtype == np.float32
        assert ("ln.weight" in sd) == (kind == "ppo")
        assert sd["encoder.fc1.weight"].shape == (64, o * s) and sd["fc_mu.weight"].shape == (a, 64)


@pytest.mark.parametrize("kind,o,a,s", CASES)
def test_model_is_as_close_to_float64_as_the_reference(kind, o, a, s):
    z, sd, mu, pre, std = load(kind, o, a, s)
    for name, mine in (("mu", mu), ("std", std)):
        e_ref = np.max(np.abs(z[name + "32"].astype(np.float64) - z[name + "64"]))
        e_model = np.max(np.abs(mine.astype(np.float64) - z[name + "64"]))
        print(f"{kind} ({o}, {a}, {s}) {name}: model {e_model:.3e}  reference {e_ref:.3e}  ratio {e_model / e_ref:.2f}")
        assert e_ref > 0
        assert e_model <= MARGIN * e_ref, (name, e_model, e_ref)


@pytest.mark.parametrize("kind,o,a,s", CASES)
def test_deterministic_action(kind, o, a, s):
    z, sd, mu, pre, std = load(kind, o, a, s)
    md = float(z["max_delta"])
    raw, _ = am.act_tail(kind, mu, std, np.zeros_like(mu), am.widths(z["x"], a), z["act_low"], z["act_high"], delta_actions=True,
                         max_delta=md, deterministic=True)
    if kind == "ppo":
        assert np.array_equal(raw, np.clip(mu, np.float32(-md), np.float32(md)))
        # the reference's own clamp of its own mu: both are within their margins of the float64 mu (clamp is 1-Lipschitz)
        e_ref = np.max(np.abs(z["mu32"].astype(np.float64) - z["mu64"]))
        assert np.max(np.abs(raw.astype(np.float64) - z["action"])) <= (MARGIN + 1) * e_ref
    else:
        e_ref = np.max(np.abs(z["mu32"].astype(np.float64) - z["mu64"]))
        # tanh is 1-Lipschitz, so the margin of mu carries over scaled by max_delta; 2 ulps for the rounding of tanh and of the product
        bound = md * MARGIN * e_ref + 2 * am.ulp(z["action"])
        assert np.all(np.abs(raw.astype(np.float64) - z["action"]) <= bound)
        assert np.all(np.abs(raw.astype(np.float64) - np.tanh(z["mu64"]) * md) <= bound)


def test_input_permutation():
    """Input i = f * S + s is x[b, s, f]: an identity-like first layer hands input o to neuron o."""
    S, obs_w = 4, 6
    x = (np.arange(S * obs_w, dtype=np.float32).reshape(1, S, obs_w) + 1) * np.float32(0.5)      # x[0, s, f] = (s * obs_w + f + 1) / 2
    flat = am.flatten_stack(x)
    for f in range(obs_w):
        for s in range(S):
            assert flat[0, f * S + s] == x[0, s, f]
    w1 = np.zeros((64, S * obs_w), dtype=np.float32)
    w1[np.arange(S * obs_w), np.arange(S * obs_w)] = 1
    h = am.linear(w1, np.zeros(64, dtype=np.float32), flat)
    assert np.array_equal(h[0, :S * obs_w], np.swapaxes(x, 1, 2).reshape(-1)) and not h[0, S * obs_w:].any()
    # through the whole model: fc2 / fc identities, fc_mu picks neuron 5 = (f 1, s 1)
    eye = np.eye(64, dtype=np.float32)
    sd = {"encoder.fc1.weight": w1, "encoder.fc1.bias": np.zeros(64, np.float32), "encoder.fc2.weight": eye, "encoder.fc2.bias": np.zeros(64, np.float32),
          "fc.weight": eye, "fc.bias": np.zeros(64, np.float32), "fc_mu.weight": eye[5:6], "fc_mu.bias": np.zeros(1, np.float32),
          "fc_std.weight": eye[6:7], "fc_std.bias": np.zeros(1, np.float32)}
    mu, pre, std = am.forward("sac", sd, x)
    assert mu[0, 0] == x[0, 1, 1] and pre[0, 0] == x[0, 2, 1]


def test_accumulation_order_and_bias():
    """One accumulator that starts at the bias, k ascending: 2^24 + 1 + 1 - 2^24 in float32 is 0, any other order gives 1 or 2."""
    w = np.array([[1, 1, -1]], dtype=np.float32)
    x = np.array([[1, 1, 2.0 ** 24]], dtype=np.float32)
    assert am.linear(w, np.array([2.0 ** 24], dtype=np.float32), x)[0, 0] == 0.0


def test_layer_norm_and_softplus():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((5, 64)) * 4).astype(np.float32)
    g, b = rng.standard_normal(64).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    x64 = x.astype(np.float64)
    ref = (x64 - x64.mean(1, keepdims=True)) / np.sqrt(x64.var(1, keepdims=True) + 1e-5) * g + b
    assert np.max(np.abs(am.layer_norm(x, g, b) - ref)) < 1e-5
    z = np.array([-100, -1, 0, 1, 19.999, 20, 20.001, 50, np.nan], dtype=np.float32)
    sp = am.softplus(z)
    assert sp[5] == np.float32(np.log1p(np.exp(20.0))) and sp[6] == z[6] and sp[7] == 50 and np.isnan(sp[8]) and sp[0] > 0
    assert am.relu(np.array([-0.0], dtype=np.float32)).view(np.uint32)[0] == 0x80000000 and np.isnan(am.relu(np.array([np.nan], dtype=np.float32)))[0]


# ---------------------------------------------------------------------------------------------------- noise
def test_noise_philox_is_the_contracts():
    for g, c, d, seed in ((0, 0, 0, 7), (4095, 7, 3, 7), (17, 2, 2 ** 32 + 5, 0x1234567890)):
        w = rng_contract.philox4x32_10((g, d & 0xFFFFFFFF, 0x72 | (c << 8), d >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        mine = am.philox4x32_10((g, d & 0xFFFFFFFF, 0x72 | (c << 8), d >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert tuple(int(v) for v in mine) == tuple(w)
        u1, u2 = (w[0] + 1) * 2.0 ** -32, w[1] * 2.0 ** -32
        assert am.noise(seed, g, c, d) == np.float32(np.sqrt(-2 * np.log(u1)) * np.cos(6.283185307179586 * u2))


def test_noise_is_standard_normal():
    from scipy import stats

    eps = am.noise(7, np.arange(4096)[:, None], np.arange(8)[None, :], 0).astype(np.float64).reshape(-1)
    n = eps.size
    assert n == 32768 and np.all(np.isfinite(eps))
    print(f"mean {eps.mean():.5f} (bound {5 / np.sqrt(n):.5f})  var {eps.var():.5f} (bound 1 +- {5 * np.sqrt(2 / n):.5f})  "
          f"KS p {stats.kstest(eps, 'norm').pvalue:.4f}")
    assert abs(eps.mean()) <= 5 / np.sqrt(n)
    assert abs(eps.var() - 1) <= 5 * np.sqrt(2 / n)
    assert stats.kstest(eps, "norm").pvalue > 1e-4


def test_noise_streams_are_distinct():
    g, c, d = np.meshgrid(np.arange(6), np.arange(8), np.arange(5), indexing="ij")
    eps = am.noise(7, g, c, d).reshape(-1)
    assert len(set(eps.view(np.uint32).tolist())) == eps.size
    assert am.noise(7, 3, 2, 1) != am.noise(7, 3, 2, 1 + 2 ** 32)
    assert am.noise(7, 3, 2, 1) != am.noise(8, 3, 2, 1)
