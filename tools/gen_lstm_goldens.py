"""Record what the reference's PPOAgent computes with its LSTM networks (its default use_stacked_obs=False) for one trajectory per case:
tests/golden/lstm_<case>.npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  rl.agents.PPO_org is imported the way tools/gen_actor_goldens.py imports it.  The
reference's own PPOAgent(use_delta_actions=True) is constructed and fed a trajectory the way its training loop feeds it: reset_buffer(),
then per step its stateful take_action on the single observation and store_transition of the observation, the clamped delta, the next
observation, the reward and done.  Then its own value_net.forward_all_steps, actor, Normal.log_prob and rl_utils.compute_gae are CALLED on
the stored lists as update() calls them (PPO_org.py:540-577), in float32 and again with the modules converted to float64; only inputs and
recorded results are stored:

    actor.<key>, value.<key>     the state dicts (float32): lstm.weight_ih_l0 / weight_hh_l0 / bias_ih_l0 / bias_hh_l0, mean_head, std_head,
                                 value_head
    obs [T + 1, obs_dim]         float32, N(0, 3^2) with +-0.0 mixed in; row 0 is the reset observation
    actions [T, act_dim]         float32, what take_action returned (the clamped delta)
    rewards [T], dones [T]       float32; dones is 0 except the last row (1)
    <out>32, <out>64             values [T], next_values [T] (forward_all_steps of the next states from hidden = None: a run of its own),
                                 mu, std, old_log_probs [T, act_dim], td_target [T], advantage [T] (the raw compute_gae result), and
                                 td_target_open / advantage_open: the same trajectory with the last row NOT done
    det_actions [T, act_dim]     take_action(obs[t], deterministic=True), t = 0 .. T - 1, stepwise from a fresh hidden state
    gamma, lmbda, max_delta, info_json

As a cross-check the agent's own update() runs with epochs = 0 and a recording wrapper around the compute_gae name of its module: the
td_delta it formed must equal the tool's float32 td_target - values bit for bit.

Cases: (obs_dim, act_dim, weight scale) in (4, 1, 1), (20, 4, 3), (56, 8, 3), (6, 2, 1).  T = 37.  The tool asserts 0.05 <= std <= 10:
below that the reference's own float32 log-probability loses whole digits and a comparison against float64 would check nothing (DESIGN
section 15); a case that violates it gets another seed (SEEDS), never another bound.

    python tools/gen_lstm_goldens.py
"""
import copy
import json
import os
import sys

# MKL's strict reproducibility mode, set before torch loads MKL (tools/gen_ppo_eval_goldens.py)
os.environ.setdefault("MKL_CBWR", "AVX2,STRICT")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_harness as rh  # noqa: E402,F401  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

from gen_actor_goldens import modules  # noqa: E402
from gen_ppo_eval_goldens import gae64  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ((4, 1, 1.0), (20, 4, 3.0), (56, 8, 3.0), (6, 2, 1.0))     # obs_dim, act_dim, weight scale
SEEDS = (900, 901, 902, 903)                                       # torch.manual_seed per case
T, MAX_DELTA = 37, 2.5
OUTPUTS = ("values", "next_values", "mu", "std", "old_log_probs", "td_target", "advantage", "td_target_open", "advantage_open")


def pipeline(torch, rl_utils, actor, value_net, gamma, lmbda, states, next_states, actions, rewards, dones):
    """PPO_org.py:540-577 line by line (the LSTM branches, without the advantage normalisation), for dones and for the variant with
    the last row open."""
    from torch.distributions import Normal

    states_seq, next_states_seq = states.unsqueeze(0), next_states.unsqueeze(0)
    next_values, _ = value_net.forward_all_steps(next_states_seq)
    next_values = next_values.squeeze(0)
    values, _ = value_net.forward_all_steps(states_seq)
    values = values.squeeze(0)
    out = dict(values=values[:, 0], next_values=next_values[:, 0])
    open_dones = dones.clone()
    open_dones[-1] = 0
    for tag, d in (("", dones), ("_open", open_dones)):
        td_target = rewards + gamma * next_values * (1 - d)
        td_delta = td_target - values
        out["td_target" + tag] = td_target[:, 0]
        single = td_delta.dtype == torch.float32
        out["advantage" + tag] = (rl_utils.compute_gae(gamma, lmbda, td_delta.cpu()) if single else gae64(gamma, lmbda, td_delta))[:, 0]
    mu, std, _ = actor(states_seq)
    mu, std = mu.squeeze(0), std.squeeze(0)
    out.update(mu=mu, std=std, old_log_probs=Normal(mu, std).log_prob(actions))
    return out


def record(obs_dim, act_dim, scale, k):
    import torch

    _, ppo = modules()
    rl_utils = sys.modules["rl.rl_utils"]
    torch.manual_seed(SEEDS[k])
    rng = np.random.default_rng(13000 + k)
    low, high = np.zeros(act_dim, dtype=np.float32), np.full(act_dim, 4.0, dtype=np.float32)
    agent = ppo.PPOAgent(obs_dim, act_dim, low, high, use_delta_actions=True, max_delta=MAX_DELTA)
    assert not agent.use_stacked_obs and type(agent.actor).__name__ == "LSTMPolicyNetwork" and type(agent.value_net).__name__ == "LSTMValueNetwork"
    with torch.no_grad():
        for net in (agent.actor, agent.value_net):
            for p in net.parameters():
                p.mul_(scale)
    obs = (rng.standard_normal((T + 1, obs_dim)) * 3.0).astype(np.float32)
    pick = rng.integers(0, 16, size=obs.shape)
    obs[pick == 0] = 0.0
    obs[pick == 1] = -0.0
    rewards = rng.standard_normal(T).astype(np.float32)
    dones = np.zeros(T, dtype=np.float32)
    dones[-1] = 1.0

    # the training loop's feeding: the agent's own hidden state runs through take_action
    agent.reset_buffer()
    actions = []
    with torch.no_grad():
        for t in range(T):
            action = agent.take_action(obs[t])
            agent.store_transition(state=obs[t], action=action, next_state=obs[t + 1], reward=rewards[t], done=bool(dones[t]))
            actions.append(np.asarray(action, dtype=np.float32).reshape(act_dim))
    actions = np.stack(actions)
    assert np.abs(actions).max() <= MAX_DELTA

    td = agent.transition_dict
    states = torch.tensor(np.array(td["states"]), dtype=torch.float)
    next_states = torch.tensor(np.array(td["next_states"]), dtype=torch.float)
    acts = torch.tensor(np.array(td["actions"])).view(-1, act_dim)
    r = torch.tensor(np.array(td["rewards"]), dtype=torch.float).view(-1, 1)
    d = torch.tensor(np.array(td["dones"]), dtype=torch.float).view(-1, 1)
    assert acts.dtype == torch.float32 and np.array_equal(acts.numpy(), actions)
    with torch.no_grad():
        out32 = pipeline(torch, rl_utils, agent.actor, agent.value_net, agent.gamma, agent.lmbda, states, next_states, acts, r, d)
        dbl = lambda m: copy.deepcopy(m).double()
        out64 = pipeline(torch, rl_utils, dbl(agent.actor), dbl(agent.value_net), agent.gamma, agent.lmbda, states.double(),
                         next_states.double(), acts.double(), r.double(), d.double())

    # the agent's own update() with no epochs: the td_delta it hands to compute_gae
    seen = []
    real = ppo.compute_gae

    def recording(gamma, lmbda, td_delta):
        seen.append(td_delta.clone())
        return real(gamma, lmbda, td_delta)

    ppo.compute_gae = recording
    try:
        agent.epochs = 0
        agent.update()
    finally:
        ppo.compute_gae = real
    mine = (out32["td_target"] - out32["values"]).view(-1, 1)
    assert len(seen) == 1 and seen[0].dtype == torch.float32 and torch.equal(seen[0], mine), "the pipeline is not update()'s"

    # stepwise and deterministic, from a fresh hidden state
    agent.reset_buffer()
    with torch.no_grad():
        det = np.stack([np.asarray(agent.take_action(obs[t], deterministic=True), dtype=np.float32).reshape(act_dim) for t in range(T)])

    std32 = out32["std"].numpy()
    assert 0.05 <= std32.min() and std32.max() <= 10.0, (std32.min(), std32.max())

    sd = lambda m: {key: v.detach().numpy().astype(np.float32).copy() for key, v in m.state_dict().items()}
    out = {}
    for tag, m in (("actor", agent.actor), ("value", agent.value_net)):
        out.update({f"{tag}.{key}": v for key, v in sd(m).items()})
    for name in OUTPUTS:
        assert out32[name].dtype == torch.float32 and out64[name].dtype == torch.float64, name
        out[name + "32"], out[name + "64"] = out32[name].numpy(), out64[name].numpy()
    info = {"obs_dim": obs_dim, "act_dim": act_dim, "scale": scale, "T": T, "seed": SEEDS[k], "std_min": float(std32.min()),
            "std_max": float(std32.max()), "numpy": np.__version__, "torch": torch.__version__, "MKL_CBWR": os.environ["MKL_CBWR"]}
    out.update(obs=obs, actions=actions, rewards=rewards, dones=dones, det_actions=det, gamma=np.float64(agent.gamma),
               lmbda=np.float64(agent.lmbda), max_delta=np.float64(MAX_DELTA), info_json=np.array(json.dumps(info)))
    path = os.path.join(GOLDEN, f"lstm_o{obs_dim}_a{act_dim}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes  std in [{std32.min():.3g}, {std32.max():.3g}]  "
          f"logp32 error {np.max(np.abs(out['old_log_probs32'] - out['old_log_probs64'])):.2e}  "
          f"value32 error {np.max(np.abs(out['values32'] - out['values64'])):.2e}", flush=True)


if __name__ == "__main__":
    for k, (obs_dim, act_dim, scale) in enumerate(CASES):
        record(obs_dim, act_dim, scale, k)
