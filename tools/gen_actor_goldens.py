"""Record what the reference's stacked actors compute for a few random stacks: tests/golden/actor_<case>.npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  rl.agents.SAC and rl.agents.PPO_org are imported under the bare `rl` package of
oracle/ref_harness.load_reference_rl(); PPO_org's import line of torch_geometric (used by its GAT actor only) is satisfied with empty
stand-in modules.  The reference's own classes are constructed (SACAgent / PPOAgent with use_stacked_obs) and CALLED; only inputs and
recorded results are stored:

    sd.<key>            the actor's state_dict (float32): encoder.fc1 / encoder.fc2 / fc / fc_mu / fc_std (+ ln for PPO), .weight / .bias
    x [B, S, obs_dim]   float32, N(0, 3^2) with +-0.0 mixed in
    mu32, std32         the actor's float32 forward
    mu64, std64         the same module converted to float64, on the same inputs
    action [B, act_dim] take_action(state, deterministic=True) per sample (SAC: tanh(mu) * max_delta; PPO with delta actions: clamp(mu))
    act_low, act_high, max_delta, info_json

Cases: SAC and PPO, (obs_dim, act_dim, S) in (4, 1, 4), (20, 4, 5), (56, 8, 5), (6, 2, 1); the first and the last with the default
initialisation, the two others with every parameter multiplied by 3.  B = 64.

    python tools/gen_actor_goldens.py
"""
import importlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = ((4, 1, 4, 1.0), (20, 4, 5, 3.0), (56, 8, 5, 3.0), (6, 2, 1, 1.0))     # obs_dim, act_dim, S, weight scale
B, MAX_DELTA = 64, 2.5


def modules():
    rh.load_reference_rl()
    for name in ("torch_geometric", "torch_geometric.nn", "torch_geometric.data"):
        sys.modules.setdefault(name, types.ModuleType(name))
    # the names PPO_org's import line asks for (its stacked network uses none of them)
    sys.modules["torch_geometric.nn"].__dict__.setdefault("GATConv", object)
    sys.modules["torch_geometric.data"].__dict__.setdefault("Data", object)
    sys.modules["torch_geometric.data"].__dict__.setdefault("Batch", object)
    return importlib.import_module("rl.agents.SAC"), importlib.import_module("rl.agents.PPO_org")


def record(kind, obs_dim, act_dim, S, scale, k):
    import copy

    import torch

    sac, ppo = modules()
    torch.manual_seed(100 + k)
    rng = np.random.default_rng(7000 + k)
    low, high = np.zeros(act_dim, dtype=np.float32), np.full(act_dim, 4.0, dtype=np.float32)
    if kind == "sac":
        agent = sac.SACAgent(obs_dim, act_dim, low, high, stack_size=S, hidden_size=64, max_delta=MAX_DELTA)
    else:
        agent = ppo.PPOAgent(obs_dim, act_dim, low, high, use_delta_actions=True, max_delta=MAX_DELTA, use_stacked_obs=True,
                             stack_size=S, hidden_size=64)
    actor = agent.actor
    with torch.no_grad():
        for p in actor.parameters():
            p.mul_(scale)
    x = (rng.standard_normal((B, S, obs_dim)) * 3.0).astype(np.float32)
    pick = rng.integers(0, 16, size=x.shape)
    x[pick == 0] = 0.0
    x[pick == 1] = -0.0
    with torch.no_grad():
        mu32, std32 = actor(torch.tensor(x))
        mu64, std64 = copy.deepcopy(actor).double()(torch.tensor(x).double())
        action = np.stack([np.asarray(agent.take_action(x[b], deterministic=True), dtype=np.float32).reshape(act_dim) for b in range(B)])
    assert mu32.dtype == torch.float32 and mu64.dtype == torch.float64 and tuple(mu32.shape) == (B, act_dim)
    out = {"sd." + key: v.detach().numpy().astype(np.float32) for key, v in actor.state_dict().items()}
    out.update(x=x, mu32=mu32.numpy(), std32=std32.numpy(), mu64=mu64.numpy(), std64=std64.numpy(), action=action, act_low=low,
               act_high=high, max_delta=np.float64(MAX_DELTA),
               info_json=np.array(json.dumps({"kind": kind, "obs_dim": obs_dim, "act_dim": act_dim, "stack_size": S, "scale": scale,
                                              "numpy": np.__version__, "torch": torch.__version__})))
    path = os.path.join(GOLDEN, f"actor_{kind}_o{obs_dim}_a{act_dim}_s{S}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    for k, (obs_dim, act_dim, S, scale) in enumerate(SHAPES):
        for kind in ("sac", "ppo"):
            record(kind, obs_dim, act_dim, S, scale, 2 * k + (kind == "ppo"))
