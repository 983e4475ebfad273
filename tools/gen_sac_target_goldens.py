"""Record what the reference's SACAgent.calc_target and soft_update compute for a few random minibatches: tests/golden/sactd_<case>.npz
and tests/golden/sactd_polyak_<case>.npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  rl.agents.SAC is imported under the bare `rl` package of
oracle/ref_harness.load_reference_rl().  The reference's own SACAgent is constructed and its calc_target and soft_update are CALLED; only
inputs and recorded results are stored:

    sactd_<case>.npz
      actor.<key>, tc1.<key>, tc2.<key>   the state dicts of the actor and of the two target critics (float32)
      x [B, S, obs_dim], rewards [B], dones [B]   float32; x is N(0, 3^2) with +-0.0 mixed in, a quarter of the rows is done
      eps [B, act_dim]      the standard normal numbers Normal.rsample drew inside calc_target (torch re-seeded, the same call)
      log_alpha             float32 scalar
      <out>32, <out>64      mu, std, logp, next_actions [B, act_dim], entropy, q1, q2, td_target [B]: the reference's float32 pipeline, and
                            the same modules converted to float64 on the same inputs and eps.  td_target32 IS calc_target's own return
                            value: the tool asserts that the float32 pipeline written out here reproduces it bit for bit.
      gamma, tau, max_delta, info_json
    sactd_polyak_<case>.npz
      c1.<key>, c2.<key>    the online critics;  after1.<key>, after2.<key>  the target critics behind ONE soft_update each

Cases: (obs_dim, act_dim, S) in (4, 1, 4), (20, 4, 5), (56, 8, 5), (6, 2, 1) with log_alpha log 0.01, 0.3, -1.0, log 0.01; the first and
the last with the default initialisation, the two others with every parameter multiplied by 3 except fc_std.weight, which gets 1 / 27:
multiplying it by 3 as well drives std below 1e-4, where the reference's own float32 log-probability is off by whole units and a
comparison against float64 would check nothing.  The tool asserts 0.05 <= std <= 20.  target_critic_2 is perturbed so that the minimum
switches between the critics.  B = 256.

    python tools/gen_sac_target_goldens.py
"""
import copy
import importlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# obs_dim, act_dim, S, weight scale, log_alpha
SHAPES = ((4, 1, 4, 1.0, math.log(0.01)), (20, 4, 5, 3.0, 0.3), (56, 8, 5, 3.0, -1.0), (6, 2, 1, 1.0, math.log(0.01)))
B, MAX_DELTA = 256, 2.5
OUTPUTS = ("mu", "std", "logp", "next_actions", "entropy", "q1", "q2", "td_target")


def pipeline(torch, actor, tc1, tc2, log_alpha, gamma, bound, rewards, ns, dones, eps):
    """calc_target (SAC.py:296-312) line by line with the drawn numbers handed in: Normal.rsample is loc + eps * scale."""
    from torch.distributions import Normal

    mu, std = actor(ns)
    dist = Normal(mu, std)
    normal_sample = mu + eps * std
    logp = dist.log_prob(normal_sample)
    na = torch.tanh(normal_sample)
    logp = logp - torch.log(1 - torch.tanh(na).pow(2) + 1e-7)
    na = na * bound
    entropy = -logp.sum(dim=1, keepdim=True)
    q1, q2 = tc1(ns, na), tc2(ns, na)
    nv = torch.min(q1, q2) + log_alpha.exp() * entropy
    td = rewards + gamma * nv * (1 - dones)
    return dict(mu=mu, std=std, logp=logp, next_actions=na, entropy=entropy[:, 0], q1=q1[:, 0], q2=q2[:, 0], td_target=td[:, 0])


def record(obs_dim, act_dim, S, scale, log_alpha, k):
    import torch
    from torch.distributions.utils import _standard_normal

    rh.load_reference_rl()
    sac = importlib.import_module("rl.agents.SAC")
    torch.manual_seed(300 + k)
    rng = np.random.default_rng(9000 + k)
    low, high = np.zeros(act_dim, dtype=np.float32), np.full(act_dim, 4.0, dtype=np.float32)
    agent = sac.SACAgent(obs_dim, act_dim, low, high, stack_size=S, hidden_size=64, max_delta=MAX_DELTA)
    with torch.no_grad():
        for net in (agent.actor, agent.critic_1, agent.critic_2):
            for name, p in net.named_parameters():
                p.mul_(scale if not (name == "fc_std.weight" and scale != 1.0) else 1.0 / 27.0)
        agent.target_critic_1.load_state_dict(agent.critic_1.state_dict())
        agent.target_critic_2.load_state_dict(agent.critic_2.state_dict())
        for p in agent.target_critic_1.parameters():          # the targets lag behind the online critics
            p.mul_(1 + 0.05 * torch.randn_like(p))
        for p in agent.target_critic_2.parameters():
            p.mul_(1 + 0.3 * torch.randn_like(p))
    agent.log_alpha = torch.tensor(log_alpha, dtype=torch.float)

    x = (rng.standard_normal((B, S, obs_dim)) * 3.0).astype(np.float32)
    pick = rng.integers(0, 16, size=x.shape)
    x[pick == 0] = 0.0
    x[pick == 1] = -0.0
    rewards = rng.standard_normal(B).astype(np.float32)
    dones = (rng.integers(0, 4, size=B) == 0).astype(np.float32)
    ns, r, d = torch.tensor(x), torch.tensor(rewards).view(-1, 1), torch.tensor(dones).view(-1, 1)
    with torch.no_grad():
        torch.manual_seed(500 + k)
        td_ref = agent.calc_target(r, ns, d)                  # the reference's own call
        torch.manual_seed(500 + k)
        mu, _ = agent.actor(ns)
        eps = _standard_normal(mu.shape, dtype=mu.dtype, device=mu.device)       # the call Normal.rsample makes
        out32 = pipeline(torch, agent.actor, agent.target_critic_1, agent.target_critic_2, agent.log_alpha, agent.gamma, agent.action_bound,
                         r, ns, d, eps)
        assert td_ref.dtype == torch.float32 and torch.equal(td_ref[:, 0], out32["td_target"]), "the pipeline is not calc_target's"
        dbl = lambda m: copy.deepcopy(m).double()
        out64 = pipeline(torch, dbl(agent.actor), dbl(agent.target_critic_1), dbl(agent.target_critic_2), agent.log_alpha.double(), agent.gamma,
                         agent.action_bound, r.double(), ns.double(), d.double(), eps.double())
    std32 = out32["std"].numpy()
    assert 0.05 <= std32.min() and std32.max() <= 20.0, (std32.min(), std32.max())
    lower = (out32["q2"] < out32["q1"]).numpy()
    assert lower.any() and not lower.all(), "the minimum does not switch between the critics"

    sd = lambda m: {key: v.detach().numpy().astype(np.float32).copy() for key, v in m.state_dict().items()}
    out = {}
    for tag, m in (("actor", agent.actor), ("tc1", agent.target_critic_1), ("tc2", agent.target_critic_2)):
        out.update({f"{tag}.{key}": v for key, v in sd(m).items()})
    for name in OUTPUTS:
        assert out32[name].dtype == torch.float32 and out64[name].dtype == torch.float64
        out[name + "32"], out[name + "64"] = out32[name].numpy(), out64[name].numpy()
    info = {"obs_dim": obs_dim, "act_dim": act_dim, "stack_size": S, "scale": scale, "log_alpha": log_alpha, "std_min": float(std32.min()),
            "std_max": float(std32.max()), "q2_lower_rows": int(lower.sum()), "numpy": np.__version__, "torch": torch.__version__}
    out.update(x=x, rewards=rewards, dones=dones, eps=eps.numpy(), log_alpha=np.float32(agent.log_alpha.item()), gamma=np.float64(agent.gamma),
               tau=np.float64(agent.tau), max_delta=np.float64(MAX_DELTA), info_json=np.array(json.dumps(info)))
    case = f"o{obs_dim}_a{act_dim}_s{S}"
    path = os.path.join(GOLDEN, f"sactd_{case}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes  std in [{std32.min():.3g}, {std32.max():.3g}]  q2 lower in {lower.sum()} rows  "
          f"logp32 error {np.max(np.abs(out['logp32'] - out['logp64'])):.2e}", flush=True)

    pol = {}
    for tag, m in (("c1", agent.critic_1), ("c2", agent.critic_2)):
        pol.update({f"{tag}.{key}": v for key, v in sd(m).items()})
    agent.soft_update(agent.critic_1, agent.target_critic_1)
    agent.soft_update(agent.critic_2, agent.target_critic_2)
    for tag, m in (("after1", agent.target_critic_1), ("after2", agent.target_critic_2)):
        pol.update({f"{tag}.{key}": v for key, v in sd(m).items()})
    path = os.path.join(GOLDEN, f"sactd_polyak_{case}.npz")
    np.savez_compressed(path, **pol)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    for k, (obs_dim, act_dim, S, scale, log_alpha) in enumerate(SHAPES):
        record(obs_dim, act_dim, S, scale, log_alpha, k)
