"""The reference's stacked actors on the device: every agent's four 64-wide layers, the noise, the squashing and the delta / clip of the
training loops, for all envs and all agents in ONE launch (rl/agents/SAC.py:72-107,277-293 and :171-180; rl/agents/PPO_org.py:145-172,
470-516; pednstream_amd/csrc/pedn_actor.hpp; the contract is DESIGN section 14, tests/actor_model.py restates it in numpy).

    buf = env.replay_store(capacity, stack_size=5)
    actors = env.stacked_actors(kind="sac", stack_size=5)
    for aid in env.possible_agents:
        actors.bind(aid, my_actor_module[aid])                 # the module's parameters now live in the pack the kernel reads
    roll = env.capture(lambda obs: actors.act(buf.stacked_obs()), on_step=lambda obs, rew: buf.push(actors.actions))

``StackedActors`` is the constructor on plain numbers (no env).  Training (backward, the optimiser) stays in torch.
"""
import ctypes as C

import numpy as np

from . import engine as _engine
from . import packs

HIDDEN = 64
MAX_ACT_W = 8
TABLE_COLS = 6                  # obs0, obs_w, act0, act_w, parameter offset (floats), reserved
KINDS = {"sac": 0, "ppo": 1}
MODES = {"draw": 0, "given": 1, "deterministic": 2}


def tensor_shapes(kind, obs_w, act_w, stack_size, hidden_size=HIDDEN):
    """[(state_dict key, shape)] of one agent in the order of the pack."""
    h = int(hidden_size)
    out = [("encoder.fc1.weight", (h, int(stack_size) * int(obs_w))), ("encoder.fc1.bias", (h,)),
           ("encoder.fc2.weight", (h, h)), ("encoder.fc2.bias", (h,)), ("fc.weight", (h, h)), ("fc.bias", (h,))]
    if kind == "ppo":
        out += [("ln.weight", (h,)), ("ln.bias", (h,))]
    return out + [("fc_mu.weight", (int(act_w), h)), ("fc_mu.bias", (int(act_w),)), ("fc_std.weight", (int(act_w), h)), ("fc_std.bias", (int(act_w),))]


def pack_layout(kind, agents, stack_size, hidden_size=HIDDEN):
    """(offsets, total): offsets[i] = {key: (offset in floats, shape)} of agent i = (obs0, obs_w, act0, act_w), one agent behind the
    other; every agent starts on a multiple of 4 floats."""
    return packs.layout([tensor_shapes(kind, obs_w, act_w, stack_size, hidden_size) for (_, obs_w, _, act_w) in agents], round_total=False)


def agent_table(kind, agents, stack_size):
    """int32 [n_agents, TABLE_COLS] the kernel reads."""
    offsets, _ = pack_layout(kind, agents, stack_size)
    return np.array([[o0, ow, a0, aw, off["encoder.fc1.weight"][0], 0] for (o0, ow, a0, aw), off in zip(agents, offsets)], dtype=np.int32)


def make_module(kind, obs_w, act_w, stack_size, min_std=1e-3, max_std=10.0):
    """A torch module with the reference actor's layers, parameter names and forward (``forward(x [B, S, obs_w]) -> mu, std``), for
    training beside the kernel: ``StackedActors.bind`` makes its parameters views of the pack."""
    import torch
    from torch import nn

    if kind not in KINDS:
        raise ValueError(f"kind must be 'sac' or 'ppo', got {kind!r}")

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder, self.fc = packs.make_encoder(obs_w, stack_size), nn.Linear(HIDDEN, HIDDEN)
            if kind == "ppo":
                self.ln = nn.LayerNorm(HIDDEN)
            self.fc_mu, self.fc_std = nn.Linear(HIDDEN, int(act_w)), nn.Linear(HIDDEN, int(act_w))

        def forward(self, x):
            h = self.fc(self.encoder(x.transpose(1, 2).flatten(1)))       # input f * S + s is x[b, s, f]
            h = torch.relu(self.ln(h) if kind == "ppo" else h)
            std = nn.functional.softplus(self.fc_std(h))
            return self.fc_mu(h), (std.clamp(min_std, max_std) if kind == "ppo" else std)

    return Actor()


class StackedActors:
    """``agents``: [(obs0, obs_w, act0, act_w)] column ranges of each agent in an observation row of ``n_obs`` floats and an action row of
    ``n_actions``; ``low`` / ``high`` [n_actions] the bounds of the absolute actions; ``agent_ids`` names them (default 0, 1, ...)."""

    def __init__(self, kind, agents, low, high, n_envs, n_obs, n_actions, stack_size=4, delta_actions=True, max_delta=2.5, min_std=1e-3,
                 max_std=10.0, seed=0, replica_offset=0, device=0, hidden_size=HIDDEN, agent_ids=None):
        if kind not in KINDS:
            raise ValueError(f"kind must be 'sac' or 'ppo', got {kind!r}")
        if int(hidden_size) != HIDDEN:
            raise ValueError(f"the actor kernel is built for hidden_size {HIDDEN}, got {hidden_size}")
        if int(stack_size) < 1:
            raise ValueError(f"stack_size must be positive, got {stack_size}")
        if int(n_envs) < 1 or int(n_obs) < 1 or int(n_actions) < 1:
            raise ValueError("n_envs, n_obs and n_actions must be positive")
        agents = [tuple(int(v) for v in a) for a in agents]
        if not agents or len(agents) > 65535 or any(len(a) != 4 for a in agents):
            raise ValueError("agents must be a non-empty list of (obs0, obs_w, act0, act_w)")
        self.kind, self.n_envs, self.n_obs, self.n_actions, self.stack_size = kind, int(n_envs), int(n_obs), int(n_actions), int(stack_size)
        self.delta_actions, self.max_delta, self.min_std, self.max_std = bool(delta_actions), float(max_delta), float(min_std), float(max_std)
        self.seed, self.replica_offset, self.device = int(seed), int(replica_offset), int(device)
        if not (0 <= self.replica_offset and self.replica_offset + self.n_envs <= 2 ** 32) or not 0 <= self.seed < 2 ** 64:
            raise ValueError("replica_offset + n_envs must fit 32 bits and the seed 64")
        if not (self.max_delta > 0 and 0 < self.min_std <= self.max_std):
            raise ValueError("max_delta must be positive and 0 < min_std <= max_std")
        covered = np.zeros(self.n_actions, dtype=np.int32)
        for (o0, ow, a0, aw) in agents:
            if not (ow >= 1 and o0 >= 0 and o0 + ow <= self.n_obs):
                raise ValueError(f"observation columns [{o0}, {o0 + ow}) are not inside a row of {self.n_obs}")
            if not (1 <= aw <= MAX_ACT_W):
                raise ValueError(f"an agent has 1 to {MAX_ACT_W} actions, got {aw}")
            if not (a0 >= 0 and a0 + aw <= self.n_actions):
                raise ValueError(f"action columns [{a0}, {a0 + aw}) are not inside a row of {self.n_actions}")
            if self.delta_actions and ow % aw:
                raise ValueError(f"delta actions read the last of obs_w / act_w features per action: {ow} is no multiple of {aw}")
            covered[a0:a0 + aw] += 1
        if covered.max() > 1:
            raise ValueError("two agents write the same action column")
        self.low, self.high = (np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (low, high))
        if self.low.shape != (self.n_actions,) or self.high.shape != (self.n_actions,) or not np.all(self.low <= self.high):
            raise ValueError(f"low and high must be [{self.n_actions}] with low <= high")
        self.agents = agents
        self.agent_ids = list(agent_ids) if agent_ids is not None else list(range(len(agents)))
        if len(self.agent_ids) != len(agents) or len(set(self.agent_ids)) != len(agents):
            raise ValueError("agent_ids must name every agent once")
        self.offsets, self.pack_size = pack_layout(kind, agents, self.stack_size)
        self.table = agent_table(kind, agents, self.stack_size)
        self._loaded = set()
        self._dev = None               # the device tensors, allocated once (a captured graph owns their addresses)

    # ------------------------------------------------------------------------------------------------ parameters
    def _index(self, agent_id):
        return packs.index(self.agent_ids, agent_id)

    def _device(self):
        if self._dev is None:
            import torch

            dev = torch.device("cuda", self.device)
            z = lambda dtype: torch.zeros(self.n_envs, self.n_actions, dtype=dtype, device=dev)
            self._dev = {"pack": torch.zeros(max(1, self.pack_size), dtype=torch.float32, device=dev),
                         "table": torch.as_tensor(self.table, device=dev), "low": torch.as_tensor(self.low, device=dev),
                         "high": torch.as_tensor(self.high, device=dev), "state": torch.zeros(2, dtype=torch.int64, device=dev),
                         "mu": z(torch.float32), "std": z(torch.float32), "eps": z(torch.float32), "raw": z(torch.float32),
                         "actions": z(torch.float64)}
        return self._dev

    def load_state_dict(self, agent_id, state_dict):
        """Copy an actor's tensors (the reference's keys, ``nn.Linear`` layout; torch tensors or arrays) into the pack."""
        i = self._index(agent_id)
        has_ln = any(k.startswith("ln.") for k in state_dict)
        if self.kind == "sac" and has_ln:
            raise ValueError("a state dict with ln.* belongs to the PPO kind (StackedPolicyNetwork), these actors are kind='sac'")
        if self.kind == "ppo" and not has_ln:
            raise ValueError("kind='ppo' needs the LayerNorm's ln.weight / ln.bias (StackedPolicyNetwork)")
        packs.load(self.offsets[i], state_dict, lambda: self._device()["pack"])
        self._loaded.add(i)

    def parameters(self, agent_id):
        """{key: float32 CUDA tensor} in ``nn.Linear`` shapes; the tensors ALIAS the pack the kernel reads."""
        want = self.offsets[self._index(agent_id)]
        return packs.views(self._device()["pack"], want)

    def bind(self, agent_id, module):
        """Copy the module's parameters into the pack and point every ``param.data`` at its view there: an optimiser that steps the
        module updates what the kernel reads, with no copy per update."""
        self.load_state_dict(agent_id, {k: v for k, v in module.state_dict().items()})
        packs.check_module(module, self.offsets[self._index(agent_id)])
        return packs.repoint(module, self.parameters(agent_id))

    # ------------------------------------------------------------------------------------------------ acting
    def act(self, stack, deterministic=False, noise=None):
        """``actions`` float64 [n_envs, n_actions] (the same tensor every call) for ``stack`` [n_envs, stack_size, n_obs] float32 contiguous
        CUDA (with ``stack_size == 1`` also [n_envs, n_obs]).  ``noise`` [n_envs, n_actions] float32: use it in place of a draw.  One
        launch on the current torch stream; no allocation, no synchronisation: capturable.  A draw advances ``draws()``."""
        import torch

        shape = (self.n_envs, self.stack_size, self.n_obs)
        if not isinstance(stack, torch.Tensor):
            raise ValueError("stack must be a torch tensor")
        if not stack.is_cuda or stack.device.index != self.device:
            raise ValueError(f"stack must be on cuda:{self.device}")
        if stack.dtype != torch.float32 or not stack.is_contiguous():
            raise ValueError("stack must be a contiguous float32 tensor")
        if tuple(stack.shape) != shape and not (self.stack_size == 1 and tuple(stack.shape) == (self.n_envs, self.n_obs)):
            raise ValueError(f"stack must have shape {shape}, got {tuple(stack.shape)}")
        if noise is not None and not (isinstance(noise, torch.Tensor) and noise.is_cuda and noise.device.index == self.device and
                                      noise.dtype == torch.float32 and noise.is_contiguous() and tuple(noise.shape) == (self.n_envs, self.n_actions)):
            raise ValueError(f"noise must be a contiguous float32 CUDA tensor of shape {(self.n_envs, self.n_actions)}")
        missing = [self.agent_ids[i] for i in range(len(self.agents)) if i not in self._loaded]
        if missing:
            raise ValueError(f"no parameters were loaded for {missing}: load_state_dict() or bind() first")
        d = self._device()
        mode = MODES["deterministic"] if deterministic else (MODES["given"] if noise is not None else MODES["draw"])
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = lib.pedn_actor_forward(p(stack), p(d["table"]), p(d["low"]), p(d["high"]), p(d["pack"]), p(noise) if mode == 1 else None,
                                        p(d["mu"]), p(d["std"]), p(d["eps"]), p(d["raw"]), p(d["actions"]), p(d["state"]),
                                        self.n_envs, self.stack_size, self.n_obs, self.n_actions, len(self.agents), HIDDEN, KINDS[self.kind],
                                        int(self.delta_actions), mode, self.max_delta, self.min_std, self.max_std, self.seed, self.replica_offset,
                                        C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"pedn_actor_forward failed ({rc}): {lib.pedn_last_error(None).decode()}")
        return d["actions"]

    @property
    def actions(self):
        """The float64 [n_envs, n_actions] tensor every ``act`` writes."""
        return self._device()["actions"]

    @property
    def outputs(self):
        """``mu``, ``std``, ``eps``, ``raw``: float32 [n_envs, n_actions] tensors the last ``act`` wrote."""
        d = self._device()
        return {k: d[k] for k in ("mu", "std", "eps", "raw")}

    def draws(self):
        """How many launches have drawn noise (the device counter; waits for the device)."""
        return int(self._device()["state"][0].item())


def for_env(env, kind="sac", stack_size=4, delta_actions=True, max_delta=2.5, min_std=1e-3, max_std=10.0, seed=0):
    """``StackedActors`` over the agents, slices, bounds and global env indices of a ``VecPedNetEnv``."""
    if not hasattr(env, "network") or not hasattr(env, "possible_agents") or hasattr(env, "groups"):
        raise ValueError("stacked actors belong to one VecPedNetEnv (MultiScenarioVecEnv steps separate engines)")
    agents = [(env.obs_slices[a].start, env.obs_slices[a].stop - env.obs_slices[a].start,
               env.action_slices[a].start, env.action_slices[a].stop - env.action_slices[a].start) for a in env.possible_agents]
    return StackedActors(kind, agents, env.action_low, env.action_high, env.n_envs, env.n_obs, env.n_actions, stack_size=stack_size,
                         delta_actions=delta_actions, max_delta=max_delta, min_std=min_std, max_std=max_std, seed=seed,
                         replica_offset=env.network.replica_offset, device=env.network.device, agent_ids=list(env.possible_agents))
