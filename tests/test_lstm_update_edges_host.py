"""DESIGN section 21's "Edges" on the CPU.  (a) tests/lstm_update_model.py on networks doctored to the ends of the cell
(tests/lstm_edge_cases.py: gates that are exactly 0.0 and 1.0 or subnormal, g = +-1, h' = +-0.0) against float64 and float32 torch twins
under tests/test_lstm_update_contract.py's 4x rule, pooled as that file pools.  (b) The inputs of tests/test_gpu_lstm_update_edges.py reach
the edges they are named for: a model that is WRONG at an edge (the ReLU mask passing at h' == 0, subnormal gates flushed, the std clamp or
the +-20 clamp passing its gradient) gives other bits on them, so a kernel that is wrong in that way fails the device tests, which compare
it with the right model bit for bit.
"""
import numpy as np
import pytest

import lstm_edge_cases as ec
import lstm_update_model as lum
import test_lstm_update_contract as tc

torch = pytest.importorskip("torch")

F = np.float32


# ---------------------------------------------------------------------------------------------------- (a) the doctored networks and the 4x rule
@pytest.fixture(scope="module")
def case():
    actors, values = tc.modules(3)
    for m in actors + values:
        sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.as_tensor(v) for k, v in ec.doctor(sd).items()})
    obs, act, adv, td = tc.inputs(4)
    old, _ = tc.old_log_probs(actors, obs, act, 5)
    twin = lambda dtype: tc.twin_gradients(actors, values, obs, act, old, adv, td, dtype)
    return {"actors": actors, "values": values, "obs": obs, "act": act, "adv": adv, "td": td, "old": old, "ref64": twin(torch.float64),
            "ref32": twin(torch.float32)}


@pytest.mark.parametrize("groups", [1, 2, 3, None])
def test_doctored_model_meets_the_4x_rule_against_the_float64_twin(case, groups):
    res = tc.model_gradients(case, groups)
    for i, r in enumerate(res):
        for net in ("actor", "value"):
            missed = [k for k, ok in ec.edge_conditions(r["gates"][net]).items() if not ok]
            assert not missed, (i, net, missed)
            assert ec.subnormal(r["a_" + net]).any() and any(ec.subnormal(r[net][k]).any() for k in lum.LSTM_KEYS), (i, net)
            assert all(np.isfinite(v).all() for v in r[net].values()) and np.isfinite(r["a_" + net]).all(), (i, net)
        m, r32, r64 = tc.pools(r), tc.pools(case["ref32"][i]), tc.pools(case["ref64"][i])
        for name in m:
            err, ref = np.abs(m[name] - r64[name]).max(), np.abs(r32[name] - r64[name]).max()
            print(f"doctored agent {i} groups {groups} {name}: model {err:.3e} float32 twin {ref:.3e} ratio {err / ref:.2f}")
            assert err <= 4 * ref, (i, name, err, ref)


# ---------------------------------------------------------------------------------------------------- (b) the device tests' inputs reach the edges
def device_inputs(actors, T, N, old_of, min_std, max_std):
    """what tests/test_gpu_lstm_update_edges.py hands the kernels, with the model's log-probabilities where it asks evaluate's (the two
    agree to 2 ulps, section 17)"""
    from test_gpu_lstm import AGENTS
    from test_gpu_lstm_update import setup

    c = setup()
    obs, act = c["obs"][:T + 1, :N], c["actions"][:T, :N]
    logp = lum.lm.evaluate(AGENTS, actors, [None] * len(AGENTS), obs, act, min_std, max_std)["old_log_probs"]
    return obs, act, old_of(logp), c["adv"][:T, :N], c["td"][:T, :N]


def both(monkeypatch, module, name, variant, actors, values, args, min_std=1e-3, max_std=10.0):
    """the model's result and the result with `module.name` replaced by the wrong variant"""
    from test_gpu_lstm import AGENTS

    run = lambda: lum.Epochs(AGENTS, actors, values, min_std, max_std).gradients(*args, groups=2)
    right = run()
    with monkeypatch.context() as mp:
        mp.setattr(module, name, variant)
        wrong = run()
    again = run()
    assert all(np.array_equal(a["a_actor"], b["a_actor"], equal_nan=True) for a, b in zip(right, again)), "the patch outlived its context"
    return right, wrong


def bits_differ(a, b):
    return np.asarray(a, dtype=F).tobytes() != np.asarray(b, dtype=F).tobytes()


def saturated():
    from test_gpu_lstm_update import setup

    c = setup()
    actors, values = ec.doctored(c)
    T, N = 4, 5
    return actors, values, device_inputs(actors, T, N, lambda logp: ec.shifted(logp, c["shift"][:T, :N]), 1e-3, 10.0)


def test_a_mask_that_passes_at_zero_changes_a(monkeypatch):
    actors, values, args = saturated()
    right, wrong = both(monkeypatch, lum.cm, "mask", ec.mask_passing_zero, actors, values, args)
    for i, (r, w) in enumerate(zip(right, wrong)):
        assert bits_differ(r["a_actor"], w["a_actor"]) and bits_differ(r["a_value"], w["a_value"]), i
        assert not bits_differ(r["log_probs"], w["log_probs"]), i


def test_flushed_subnormal_gates_change_a_or_a_weight_gradient(monkeypatch):
    actors, values, args = saturated()
    right, wrong = both(monkeypatch, lum.lm, "sigmoid", ec.flush_subnormals(lum.lm.sigmoid), actors, values, args)
    for i, (r, w) in enumerate(zip(right, wrong)):
        for net in ("actor", "value"):
            assert bits_differ(r["a_" + net], w["a_" + net]) or any(bits_differ(r[net][k], w[net][k]) for k in lum.LSTM_KEYS), (i, net)


def test_a_std_clamp_that_passes_its_gradient_changes_d_z(monkeypatch):
    from test_gpu_lstm_update import setup

    c = setup()
    T, N, lo, hi = 6, 13, 0.4, 1.2                 # (softplus passes 1.2 at step 5 of env 11, and lies under 0.4 from step 0 on)
    args = device_inputs(c["actors"], T, N, lambda logp: ec.shifted(logp, c["shift"][:T, :N]), lo, hi)
    right, wrong = both(monkeypatch, lum.um, "tail", ec.tail_without_ps(lum.um.tail), c["actors"], c["values"], args, lo, hi)
    std = np.concatenate([r["std"].reshape(-1) for r in right])
    assert (std == F(lo)).any() and (std == F(hi)).any() and ((std > F(lo)) & (std < F(hi))).any()
    assert any(bits_differ(r["d_z"], w["d_z"]) for r, w in zip(right, wrong))
    assert not any(bits_differ(r["d_mu"], w["d_mu"]) for r, w in zip(right, wrong))


def test_a_log_ratio_clamp_that_passes_its_gradient_changes_d_mu(monkeypatch):
    from test_gpu_lstm_update import setup

    c = setup()
    T, N = 5, 13
    args = device_inputs(c["actors"], T, N, ec.beyond_twenty, 1e-3, 10.0)
    right, wrong = both(monkeypatch, lum.um, "tail", ec.tail_without_pl(lum.um.tail), c["actors"], c["values"], args)
    for i, (r, w) in enumerate(zip(right, wrong)):
        aw = r["d_mu"].shape[1]
        step = lambda v, t: v.reshape(T, N, aw)[t]
        assert (step(r["d_mu"], 0) == 0).all() and (step(r["d_mu"], 1) == 0).all() and (step(r["d_z"], 0) == 0).all(), i
        assert bits_differ(r["d_mu"], w["d_mu"]) and (step(w["d_mu"], 0) != 0).any() and (step(w["d_mu"], 1) != 0).any(), i
        assert not bits_differ(step(r["d_mu"], 3), step(w["d_mu"], 3)), i


def test_the_clip_bound_inputs_put_ratios_on_both_bounds():
    from test_gpu_lstm import AGENTS, OWNED
    from test_gpu_lstm_update import setup

    c = setup()
    T, N = 5, 13
    obs, act, old, _, _ = device_inputs(c["actors"], T, N, ec.on_clip_bounds, 1e-3, 10.0)
    logp = lum.lm.evaluate(AGENTS, c["actors"], [None] * len(AGENTS), obs, act)["old_log_probs"]
    ratio = np.exp((logp - old).astype(np.float64)).astype(F)[:, :, OWNED]
    print("ratios exactly on 1.2:", int((ratio[0] == F(1.2)).sum()), "on 0.8:", int((ratio[1] == F(0.8)).sum()), "of", ratio[0].size)
    assert (ratio[0] == F(1.2)).any() and (ratio[1] == F(0.8)).any()
