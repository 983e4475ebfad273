"""Record what the reference's PPOAgent computes under torch.no_grad() before its epochs, for one trajectory per case:
tests/golden/ppoeval_<case>.npz.

Needs the reference tree (PEDN_REFERENCE_ROOT).  rl.agents.PPO_org is imported the way tools/gen_actor_goldens.py imports it.  The
reference's own PPOAgent(use_stacked_obs=True, use_delta_actions=True) is constructed and fed a trajectory the way its training loop
feeds it (PPO_org.py:250-318): a deque of S copies of the reset observation, one append per step, take_action on the stack,
store_transition of the stack, the clamped delta, the next stack, the reward and done.  Then its own value_net, actor, Normal.log_prob
and rl_utils.compute_gae are CALLED on the stored lists, in float32 and again with the modules converted to float64; only inputs and
recorded results are stored:

    actor.<key>, value.<key>     the state dicts (float32)
    obs [T + 1, obs_dim]         float32, N(0, 3^2) with +-0.0 mixed in; row 0 is the reset observation
    actions [T, act_dim]         float32, what take_action returned (the clamped delta)
    rewards [T], dones [T]       float32; dones is 0 except the last row (1)
    <out>32, <out>64             values [T], next_values [T], mu, std, old_log_probs [T, act_dim], td_target [T], advantage [T] (the raw
                                 compute_gae result), and td_target_open / advantage_open: the same trajectory with the last row NOT done
    gamma, lmbda, max_delta, info_json

As a cross-check the agent's own update() runs with epochs = 0 and a recording wrapper around the compute_gae name of its module: the
td_delta it formed must equal the tool's float32 td_target - values bit for bit.

Cases: (obs_dim, act_dim, S) in (4, 1, 4), (20, 4, 5), (56, 8, 5), (6, 2, 1); the first and the last with the default initialisation, the
two others with every parameter of both networks multiplied by 3 (tools/gen_actor_goldens.py).  T = 37.  The tool asserts
0.05 <= std <= 10: below that the reference's own float32 log-probability loses whole digits and a comparison against float64 would check
nothing.

    python tools/gen_ppo_eval_goldens.py
"""
import collections
import copy
import json
import os
import sys

# MKL's strict reproducibility mode, set before torch loads MKL: without it the last rows of a batched float32 GEMM go through a tail
# kernel that rounds differently, so one of the T rows of value_net(next_states) differs from its twin in value_net(states) by an ulp
# and next_values[t] == values[t + 1] would hold or not depending on the row's position in the batch.
os.environ.setdefault("MKL_CBWR", "AVX2,STRICT")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_harness as rh  # noqa: E402,F401  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

from gen_actor_goldens import SHAPES, modules  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
T, MAX_DELTA = 37, 2.5
OUTPUTS = ("values", "next_values", "mu", "std", "old_log_probs", "td_target", "advantage", "td_target_open", "advantage_open")


def pipeline(torch, rl_utils, actor, value_net, gamma, lmbda, states, next_states, actions, rewards, dones):
    """PPO_org.py:543-577 line by line (without the advantage normalisation), for dones and for the variant with the last row open."""
    from torch.distributions import Normal

    next_values, values = value_net(next_states), value_net(states)
    out = dict(values=values[:, 0], next_values=next_values[:, 0])
    open_dones = dones.clone()
    open_dones[-1] = 0
    for tag, d in (("", dones), ("_open", open_dones)):
        td_target = rewards + gamma * next_values * (1 - d)
        td_delta = td_target - values
        out["td_target" + tag] = td_target[:, 0]
        single = td_delta.dtype == torch.float32
        out["advantage" + tag] = (rl_utils.compute_gae(gamma, lmbda, td_delta.cpu()) if single else gae64(gamma, lmbda, td_delta))[:, 0]
    mu, std = actor(states)
    out.update(mu=mu, std=std, old_log_probs=Normal(mu, std).log_prob(actions))
    return out


def gae64(gamma, lmbda, td_delta):
    """compute_gae's recursion kept in float64 (the reference's function returns float32 whatever it is given)."""
    adv, carry = td_delta.clone(), 0.0
    for t in range(td_delta.shape[0] - 1, -1, -1):
        carry = gamma * lmbda * carry + td_delta[t]
        adv[t] = carry
    return adv


def record(obs_dim, act_dim, S, scale, k):
    import torch

    _, ppo = modules()
    rl_utils = sys.modules["rl.rl_utils"]
    torch.manual_seed(700 + k)
    rng = np.random.default_rng(11000 + k)
    low, high = np.zeros(act_dim, dtype=np.float32), np.full(act_dim, 4.0, dtype=np.float32)
    agent = ppo.PPOAgent(obs_dim, act_dim, low, high, use_delta_actions=True, max_delta=MAX_DELTA, use_stacked_obs=True, stack_size=S,
                         hidden_size=64)
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

    # the training loop's feeding (PPO_org.py:250-318)
    agent.reset_buffer()
    queue = collections.deque(maxlen=S)
    for _ in range(S):
        queue.append(obs[0])
    state = np.array(queue)
    actions = []
    with torch.no_grad():
        for t in range(T):
            action = agent.take_action(state)
            queue.append(obs[t + 1])
            next_state = np.array(queue)
            agent.store_transition(state=state, action=action, next_state=next_state, reward=rewards[t], done=bool(dones[t]))
            actions.append(np.asarray(action, dtype=np.float32).reshape(act_dim))
            state = next_state
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

    std32 = out32["std"].numpy()
    assert 0.05 <= std32.min() and std32.max() <= 10.0, (std32.min(), std32.max())
    assert torch.equal(out32["next_values"][:-1], out32["values"][1:]), "a row's value depends on its position in the batch"

    sd = lambda m: {key: v.detach().numpy().astype(np.float32).copy() for key, v in m.state_dict().items()}
    out = {}
    for tag, m in (("actor", agent.actor), ("value", agent.value_net)):
        out.update({f"{tag}.{key}": v for key, v in sd(m).items()})
    for name in OUTPUTS:
        assert out32[name].dtype == torch.float32 and out64[name].dtype == torch.float64, name
        out[name + "32"], out[name + "64"] = out32[name].numpy(), out64[name].numpy()
    info = {"obs_dim": obs_dim, "act_dim": act_dim, "stack_size": S, "scale": scale, "T": T, "std_min": float(std32.min()),
            "std_max": float(std32.max()), "numpy": np.__version__, "torch": torch.__version__, "MKL_CBWR": os.environ["MKL_CBWR"]}
    out.update(obs=obs, actions=actions, rewards=rewards, dones=dones, gamma=np.float64(agent.gamma), lmbda=np.float64(agent.lmbda),
               max_delta=np.float64(MAX_DELTA), info_json=np.array(json.dumps(info)))
    path = os.path.join(GOLDEN, f"ppoeval_o{obs_dim}_a{act_dim}_s{S}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {os.path.getsize(path)} bytes  std in [{std32.min():.3g}, {std32.max():.3g}]  "
          f"logp32 error {np.max(np.abs(out['old_log_probs32'] - out['old_log_probs64'])):.2e}  "
          f"value32 error {np.max(np.abs(out['values32'] - out['values64'])):.2e}", flush=True)


if __name__ == "__main__":
    for k, (obs_dim, act_dim, S, scale) in enumerate(SHAPES):
        record(obs_dim, act_dim, S, scale, k)
