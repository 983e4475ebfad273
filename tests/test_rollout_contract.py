"""The rollout contract without a GPU: tests/rollout_model.py (what the kernels of pednstream_amd/csrc/pedn_rollout.hpp must compute) IS the
reference's compute_gae and TD-target lines bit for bit (goldens gae_*.npz, recorded from the reference by tools/gen_gae_goldens.py), its
advantage normalisation agrees with the reference's line evaluated by torch in float64, and the refusals that need no device."""
import glob
import json
import os

import numpy as np
import pytest

import rollout_model as rm
from golden_util import DATA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GAE_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "gae_*.npz")))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def load_gae(case):
    z = np.load(os.path.join(GOLDEN, case + ".npz"))
    return z, json.loads(str(z["info_json"]))


def test_the_goldens_cover_what_they_should():
    seen = {(load_gae(c)[1]["T"], load_gae(c)[1]["last_done"]) for c in GAE_CASES}
    assert seen >= {(T, d) for T in (1, 2, 3, 64, 499) for d in (0, 1)}
    products = set()
    for c in GAE_CASES:
        z, info = load_gae(c)
        assert z["dones"][-1] == info["last_done"] and not z["dones"][:-1].any()
        products.add((float(z["gamma"]), float(z["lmbda"])))
    # at least one product gamma * lmbda that binary32 does not hold: rounding it twice or in binary32 would show
    assert any(float(np.float32(g * l)) != g * l for g, l in products)
    z, _ = load_gae("gae_T499_open")
    v = z["values"]
    assert (bits(v) == 0x80000000).any() and (bits(v) == 0).any() and ((np.abs(v) > 0) & (np.abs(v) < np.finfo(np.float32).tiny)).any()


@pytest.mark.parametrize("case", GAE_CASES)
def test_model_is_the_reference_bit_for_bit(case):
    z, _ = load_gae(case)
    td, adv = rm.td_and_gae(z["rewards"], z["values"], z["dones"], float(z["gamma"]), float(z["lmbda"]))
    assert np.array_equal(bits(td), bits(z["td_target"]))
    assert np.array_equal(bits(adv), bits(z["adv"]))
    # the functional form on td_delta alone, and trailing axes are independent trajectories
    delta = z["td_target"] - z["values"][:-1]
    assert np.array_equal(bits(rm.gae_from_delta(delta, float(z["gamma"]), float(z["lmbda"]))), bits(z["adv"]))
    two = rm.gae_from_delta(np.stack([delta, -delta], axis=1), float(z["gamma"]), float(z["lmbda"]))
    assert np.array_equal(bits(two[:, 0]), bits(z["adv"]))


def test_carry_is_not_masked_by_done():
    r = np.array([1.0, 2.0, 3.0], dtype=np.float32)
    v = np.zeros(4, dtype=np.float32)
    d = np.array([0.0, 1.0, 0.0], dtype=np.float32)
    _, adv = rm.td_and_gae(r, v, d, 0.5, 1.0)
    assert adv.tolist() == [1.0 + 0.5 * (2.0 + 0.5 * 3.0), 2.0 + 0.5 * 3.0, 3.0]


@pytest.mark.parametrize("shape", [(2, 1, 1), (1, 2, 3), (7, 3, 2), (30, 65, 3), (64, 130, 5), (499, 1, 2)])
def test_normalisation_model_against_torch_in_float64(shape):
    """The reference's line (PPO_org.py:567) evaluated by torch in float64 on the same advantages, per agent, rounded to float32: the
    model differs only by its binary64 summation order and by nothing else of size, so the two agree to 1 ulp of float32 at the most.
    Largest distance observed over these shapes: 0 ulp (every entry equal)."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(sum(shape))
    adv = (rng.standard_normal(shape) * rng.uniform(0.1, 30.0, size=shape[2]) + rng.uniform(-5, 5, size=shape[2])).astype(np.float32)
    mine = rm.normalize_advantages(adv)
    assert mine.dtype == np.float32 and mine.shape == shape
    worst = 0
    for a in range(shape[2]):
        x = torch.tensor(adv[:, :, a]).double()
        ref = ((x - x.mean()) / (x.std() + 1e-8)).float().numpy()
        ulp = np.spacing(np.abs(ref))
        dist = np.abs(mine[:, :, a].astype(np.float64) - ref.astype(np.float64)) / ulp
        worst = max(worst, float(dist.max()))
    print(f"normalisation model vs torch float64, shape {shape}: {worst} ulp")
    assert worst <= 1.0


def test_normalisation_needs_two_entries():
    with pytest.raises(ValueError):
        rm.normalize_advantages(np.zeros((1, 1, 3), dtype=np.float32))


def test_refusals_without_a_device():
    torch = pytest.importorskip("torch")
    import pednstream_amd
    from pednstream_amd import rollout
    from pednstream_amd.rl_env import MultiScenarioVecEnv

    assert pednstream_amd.RolloutStore is rollout.RolloutStore and pednstream_amd.gae is rollout.gae
    cpu = torch.zeros(3, 2)
    with pytest.raises(ValueError):                    # CPU tensors
        rollout.gae(cpu, torch.zeros(4, 2), cpu, 0.99, 0.95)
    with pytest.raises(ValueError):
        rollout.compute_gae(0.99, 0.95, torch.zeros(3, 2))          # not (T, 1) / (T,)
    with pytest.raises(ValueError):
        rollout.compute_gae(0.99, 0.95, torch.zeros(0, 1))
    with pytest.raises(ValueError):
        rollout.compute_gae(0.99, 0.95, torch.zeros(3, 1, dtype=torch.int64))
    with pytest.raises(ValueError):
        rollout.RolloutStore(object())
    multi = MultiScenarioVecEnv.__new__(MultiScenarioVecEnv)          # (no engine: the refusal comes first)
    with pytest.raises(ValueError):
        multi.rollout_store()


def test_compat_installs_compute_gae():
    import sys

    import pednstream_amd.compat as compat
    from pednstream_amd import rollout

    keep = {k: sys.modules.get(k) for k in list(sys.modules) if k == "rl" or k.startswith("rl.") or k == "src" or k.startswith("src.")
            or k == "handlers" or k.startswith("handlers.")}
    try:
        compat.install(force=True)
        from rl.rl_utils import compute_gae

        assert compute_gae is rollout.compute_gae
    finally:
        for k in [k for k in sys.modules if k == "rl" or k.startswith("rl.") or k == "src" or k.startswith("src.") or k == "handlers"
                  or k.startswith("handlers.")]:
            del sys.modules[k]
        sys.modules.update({k: v for k, v in keep.items() if v is not None})
