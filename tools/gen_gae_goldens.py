"""Record what the reference's compute_gae (rl/rl_utils.py:1754-1773) and the TD-target lines of its PPO update
(rl/agents/PPO_org.py:560-561) return for a few random trajectories: tests/golden/gae_<case>.npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  rl.rl_utils is loaded through oracle/ref_harness.load_reference_rl() (a bare `rl` package)
and its own compute_gae is CALLED on td_delta of shape (T, 1), the shape the reference's update hands it; td_target / td_delta are torch's
CPU float32 ops on (T, 1) tensors, as in the update.  Only inputs and recorded results are stored:

    rewards [T] f32, values [T + 1] f32 (values[t + 1] = next_values[t], values[t] = current_values[t]), dones [T] f32,
    gamma, lmbda f64, td_target [T] f32, adv [T] f32, info_json

Cases: T in {1, 2, 3, 7, 64, 499}, the last row terminated and not; values with +-0.0 and subnormals mixed in; (gamma, lmbda) whose
binary64 product is not a binary32 number.

    python tools/gen_gae_goldens.py
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LENGTHS = (1, 2, 3, 7, 64, 499)
COEFF = ((0.99, 0.95), (0.9, 0.97), (0.995, 1.0))


def draw(rng, n, scale):
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    kind = rng.integers(0, 12, size=n)
    x[kind == 0] = 0.0
    x[kind == 1] = -0.0
    tiny = (rng.integers(1, 1 << 22, size=n).astype(np.uint32) | (rng.integers(0, 2, size=n).astype(np.uint32) << 31)).view(np.float32)
    x[kind == 2] = tiny[kind == 2]                      # subnormals
    return x


def record(T, last_done, k):
    import torch

    rh.load_reference_rl()
    utils = importlib.import_module("rl.rl_utils")
    rng = np.random.default_rng(1000 * T + 10 * k + last_done)
    gamma, lmbda = COEFF[k % len(COEFF)]
    rewards, values = draw(rng, T, 3.0), draw(rng, T + 1, 20.0)
    dones = np.zeros(T, dtype=np.float32)
    dones[-1] = float(last_done)
    r, d = torch.tensor(rewards).view(-1, 1), torch.tensor(dones).view(-1, 1)
    nv, cv = torch.tensor(values[1:]).view(-1, 1), torch.tensor(values[:-1]).view(-1, 1)
    td_target = r + gamma * nv * (1 - d)                 # PPO_org.py:560-561
    td_delta = td_target - cv
    adv = utils.compute_gae(gamma, lmbda, td_delta.cpu())
    assert adv.dtype == torch.float32 and tuple(adv.shape) == (T, 1)
    name = f"gae_T{T}_{'done' if last_done else 'open'}"
    out = {"rewards": rewards, "values": values, "dones": dones, "gamma": np.float64(gamma), "lmbda": np.float64(lmbda),
           "td_target": td_target.numpy().reshape(-1), "adv": adv.numpy().reshape(-1),
           "info_json": np.array(json.dumps({"T": T, "last_done": last_done, "numpy": np.__version__, "torch": torch.__version__}))}
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    for k, T in enumerate(LENGTHS):
        for last_done in (0, 1):
            record(T, last_done, k)
