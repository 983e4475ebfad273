"""The reference's stateful LSTM PPO agents on the device (rl/agents/PPO_org.py:20-138 ``LSTMPolicyNetwork`` / ``LSTMValueNetwork``, the
agent's default ``use_stacked_obs=False``): acting for all envs and agents in ONE launch per policy step, the recurrent state kept on the
device, and the gradient-free half of ``PPOAgent.update`` (:543-577: the value LSTM over the states and over the next states, the actor
LSTM and ``Normal.log_prob``) for a whole rollout in ONE launch.  pednstream_amd/csrc/pedn_lstm.hpp; the contract is DESIGN section 17,
tests/lstm_model.py restates it in numpy.

    actors = env.lstm_actors()
    store = env.rollout_store()
    ppo = env.lstm_ppo_targets(actors)
    for aid in env.possible_agents:
        actors.bind(aid, actor[aid]); ppo.bind(aid, value_net[aid])
    roll = env.capture(lambda obs: actors.act(obs), on_step=lambda obs, rew: store.record(actors.outputs["raw"].double(), None))
    env.reset(); store.begin(); actors.reset_hidden()
    ...                                                             # the episode
    store.finish()
    res = ppo.evaluate_store(store)                                 # values, next_values, old_log_probs
    adv, td_target = ppo.compute_gae(store, res["values"], res["next_values"], 0.99, 0.95)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)                   # the reference's normalisation line stays the caller's
    ppo.update_store(store, res["old_log_probs"], adv, td_target, epochs=10)   # the clipped-loss epochs, in place in both packs

``LstmActors`` is the constructor on plain numbers (no env).  The epochs run on the device too (``epoch_update``, ``update_store``: both
forwards over every env's whole sequence, back-propagation through time, ``clip_grad_norm_``, both Adam steps and the KL early stop of
every agent in five launches per epoch, pednstream_amd/csrc/pedn_lstm_grad.hpp, DESIGN section 21, tests/lstm_update_model.py); torch
modules bound to the packs see the steps and can still run the epochs themselves.
"""
import ctypes as C

import numpy as np

from . import engine as _engine
from . import packs
from .policy import HIDDEN, MAX_ACT_W, MODES          # (the agent table and the modes are the stacked actors')
from .ppo import TILE, EpochUpdates

ROW_FLOATS = 6 * HIDDEN         # of the epochs' activations per (network, agent, row): h', c' and the gates i, f, g, o (PEDN_LG_ROW)
TAIL_PLANES = 4                 # std, d_mu, d_z, -min(surr1, surr2) per (row, action) (PEDN_LG_TAIL)

GATE_ROWS = 4 * HIDDEN          # i, f, g, o


def _lstm_shapes(obs_w, hidden_size=HIDDEN):
    h = int(hidden_size)
    return [("lstm.weight_ih_l0", (4 * h, int(obs_w))), ("lstm.weight_hh_l0", (4 * h, h)), ("lstm.bias_ih_l0", (4 * h,)), ("lstm.bias_hh_l0", (4 * h,))]


def actor_tensor_shapes(obs_w, act_w, hidden_size=HIDDEN):
    """[(state_dict key, shape)] of one actor in the order of the pack."""
    h = int(hidden_size)
    return _lstm_shapes(obs_w, h) + [("mean_head.weight", (int(act_w), h)), ("mean_head.bias", (int(act_w),)),
                                     ("std_head.weight", (int(act_w), h)), ("std_head.bias", (int(act_w),))]


def value_tensor_shapes(obs_w, hidden_size=HIDDEN):
    """[(state_dict key, shape)] of one value network in the order of the pack."""
    h = int(hidden_size)
    return _lstm_shapes(obs_w, h) + [("value_head.weight", (1, h)), ("value_head.bias", (1,))]


def actor_pack_layout(agents):
    """(offsets, total): offsets[i] = {key: (offset in floats, shape)} of the actor of agent i = (obs0, obs_w, act0, act_w), one agent
    behind the other, every agent on a multiple of 4 floats; total is a multiple of 4 (the padding is zero)."""
    return packs.layout([actor_tensor_shapes(obs_w, act_w) for (_, obs_w, _, act_w) in agents])


def value_pack_layout(agents):
    """The same for the value networks."""
    return packs.layout([value_tensor_shapes(obs_w) for (_, obs_w, _, _) in agents])


def agent_table(agents):
    """int32 [n_agents, TABLE_COLS] the kernels read."""
    offsets, _ = actor_pack_layout(agents)
    return np.array([[o0, ow, a0, aw, off["lstm.weight_ih_l0"][0], 0] for (o0, ow, a0, aw), off in zip(agents, offsets)], dtype=np.int32)


def _check_net(hidden_size, num_layers):
    if int(hidden_size) != HIDDEN:
        raise ValueError(f"the LSTM kernels are built for hidden_size {HIDDEN}, got {hidden_size}")
    if int(num_layers) != 1:
        raise ValueError(f"the LSTM kernels are built for num_layers 1, got {num_layers}")


def make_actor_module(obs_w, act_w, min_std=1e-3, max_std=10.0, hidden_size=HIDDEN, num_layers=1):
    """A torch module with the reference actor's layers, parameter names and forward (``forward(x [B, obs_w] or [B, T, obs_w], hidden=None)
    -> mu, std, hidden``; a batch here is an env), for training beside the kernels: ``LstmActors.bind`` makes its parameters views of
    the pack."""
    import torch
    from torch import nn

    _check_net(hidden_size, num_layers)

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.lstm = nn.LSTM(input_size=int(obs_w), hidden_size=HIDDEN, num_layers=1, batch_first=True)
            self.mean_head, self.std_head = nn.Linear(HIDDEN, int(act_w)), nn.Linear(HIDDEN, int(act_w))

        def forward(self, x, hidden=None):
            out, hidden = self.lstm(x.unsqueeze(1) if x.dim() == 2 else x, hidden)
            f = torch.relu(out.squeeze(1) if x.dim() == 2 else out)
            return self.mean_head(f), nn.functional.softplus(self.std_head(f)).clamp(min_std, max_std), hidden

    return Actor()


def make_value_module(obs_w, hidden_size=HIDDEN, num_layers=1):
    """The reference value network's layers, names and forward: ``forward(x [B, obs_w] or [B, T, obs_w], hidden=None) -> value of the last
    step [B, 1], hidden`` and ``forward_all_steps(x [B, T, obs_w], hidden=None) -> values [B, T, 1], hidden``."""
    import torch
    from torch import nn

    _check_net(hidden_size, num_layers)

    class Value(nn.Module):
        def __init__(self):
            super().__init__()
            self.lstm = nn.LSTM(input_size=int(obs_w), hidden_size=HIDDEN, num_layers=1, batch_first=True)
            self.value_head = nn.Linear(HIDDEN, 1)

        def forward(self, x, hidden=None):
            out, hidden = self.lstm(x.unsqueeze(1) if x.dim() == 2 else x, hidden)
            return self.value_head(torch.relu(out[:, -1, :])), hidden

        def forward_all_steps(self, x, hidden=None):
            out, hidden = self.lstm(x, hidden)
            return self.value_head(torch.relu(out)), hidden

    return Value()


def _launch_failed(name, rc):
    return (ValueError if rc == -1 else RuntimeError)(f"{name} failed ({rc}): {_engine.lib().pedn_last_error(None).decode()}")


class LstmActors:
    """``agents``: [(obs0, obs_w, act0, act_w)] column ranges of each agent in an observation row of ``n_obs`` floats and an action row of
    ``n_actions``; ``low`` / ``high`` [n_actions] the bounds of the absolute actions; ``agent_ids`` names them (default 0, 1, ...).  The
    recurrent state of every (agent, env) lives on the device and starts at zero."""

    def __init__(self, agents, low, high, n_envs, n_obs, n_actions, delta_actions=True, max_delta=2.5, min_std=1e-3, max_std=10.0, seed=0,
                 replica_offset=0, device=0, hidden_size=HIDDEN, num_layers=1, agent_ids=None):
        _check_net(hidden_size, num_layers)
        if int(n_envs) < 1 or int(n_obs) < 1 or int(n_actions) < 1:
            raise ValueError("n_envs, n_obs and n_actions must be positive")
        agents = [tuple(int(v) for v in a) for a in agents]
        if not agents or len(agents) > 65535 or any(len(a) != 4 for a in agents):
            raise ValueError("agents must be a non-empty list of (obs0, obs_w, act0, act_w)")
        self.n_envs, self.n_obs, self.n_actions = int(n_envs), int(n_obs), int(n_actions)
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
        self.offsets, self.pack_size = actor_pack_layout(agents)
        self.table = agent_table(agents)
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
            self._dev = {"pack": torch.zeros(self.pack_size, dtype=torch.float32, device=dev),
                         "table": torch.as_tensor(self.table, device=dev), "low": torch.as_tensor(self.low, device=dev),
                         "high": torch.as_tensor(self.high, device=dev), "state": torch.zeros(2, dtype=torch.int64, device=dev),
                         "hc": torch.zeros(len(self.agents), self.n_envs, 2, HIDDEN, dtype=torch.float32, device=dev),
                         "mu": z(torch.float32), "std": z(torch.float32), "eps": z(torch.float32), "raw": z(torch.float32),
                         "actions": z(torch.float64)}
        return self._dev

    def load_state_dict(self, agent_id, state_dict):
        """Copy an actor's tensors (the reference's keys, torch's layouts; torch tensors or arrays) into the pack."""
        i = self._index(agent_id)
        packs.load(self.offsets[i], state_dict, lambda: self._device()["pack"])
        self._loaded.add(i)

    def parameters(self, agent_id):
        """{key: float32 CUDA tensor} in torch's shapes; the tensors ALIAS the pack the kernels read."""
        want = self.offsets[self._index(agent_id)]
        return packs.views(self._device()["pack"], want)

    def bind(self, agent_id, module):
        """Copy the module's parameters into the pack and point every ``param.data`` at its view there: an optimiser that steps the
        module updates what the kernels read, with no copy per update."""
        packs.check_module(module, self.offsets[self._index(agent_id)])
        self.load_state_dict(agent_id, {k: v for k, v in module.state_dict().items()})
        return packs.repoint(module, self.parameters(agent_id))

    def _missing(self):
        missing = [self.agent_ids[i] for i in range(len(self.agents)) if i not in self._loaded]
        if missing:
            raise ValueError(f"no parameters were loaded for {missing}: load_state_dict() or bind() first")

    # ------------------------------------------------------------------------------------------------ acting
    def act(self, obs, deterministic=False, noise=None):
        """``actions`` float64 [n_envs, n_actions] (the same tensor every call) for ``obs`` [n_envs, n_obs] float32 contiguous CUDA; the
        recurrent state of every (agent, env) advances one step.  ``noise`` [n_envs, n_actions] float32: use it in place of a draw.  One
        launch on the current torch stream; no allocation, no synchronisation: capturable.  A draw advances ``draws()``."""
        import torch

        packs.check_tensor("obs", obs, self.device, (self.n_envs, self.n_obs))
        if noise is not None:
            packs.check_tensor("noise", noise, self.device, (self.n_envs, self.n_actions))
        self._missing()
        d = self._device()
        mode = MODES["deterministic"] if deterministic else (MODES["given"] if noise is not None else MODES["draw"])
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = lib.pedn_lstm_actor_forward(p(obs), p(d["table"]), p(d["low"]), p(d["high"]), p(d["pack"]), p(noise) if mode == 1 else None,
                                             p(d["hc"]), p(d["mu"]), p(d["std"]), p(d["eps"]), p(d["raw"]), p(d["actions"]), p(d["state"]),
                                             self.n_envs, self.n_obs, self.n_actions, len(self.agents), HIDDEN, 1, int(self.delta_actions),
                                             mode, self.max_delta, self.min_std, self.max_std, self.seed, self.replica_offset,
                                             C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise _launch_failed("pedn_lstm_actor_forward", rc)
        return d["actions"]

    def reset_hidden(self, mask=None):
        """h = c = 0 for every env, or for the envs where ``mask`` (bool or uint8 [n_envs], contiguous CUDA) is set: the reference's
        ``reset_buffer()``.  One launch on the current torch stream, capturable."""
        import torch

        if mask is not None:
            packs.check_tensor("mask", mask, self.device, (self.n_envs,), (torch.bool, torch.uint8))
        d = self._device()
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        with torch.cuda.device(self.device):
            rc = _engine.lib().pedn_lstm_reset(C.c_void_p(d["hc"].data_ptr()), C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                               self.n_envs, len(self.agents), HIDDEN, C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise _launch_failed("pedn_lstm_reset", rc)

    @property
    def hidden(self):
        """``{"h": [n_agents, n_envs, 64], "c": ...}``: float32 views of the recurrent state the launches update."""
        hc = self._device()["hc"]
        return {"h": hc[:, :, 0], "c": hc[:, :, 1]}

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


class LstmPpoTargets(EpochUpdates):
    """``actors``: a ``LstmActors``; the agent table, ``min_std`` / ``max_std`` and the device are its.  The actors' pack is read in place
    (and stepped in place by the epochs); the value networks live in a pack of their own."""

    _BEGIN = "pedn_lstm_ppo_begin_update"

    def __init__(self, actors):
        if not isinstance(actors, LstmActors):
            raise ValueError("actors must be a LstmActors")
        self.actors = actors
        self.agents, self.agent_ids, self.device = actors.agents, actors.agent_ids, actors.device
        self.n_obs, self.n_actions, self.n_agents = actors.n_obs, actors.n_actions, len(actors.agents)
        self.offsets, self.pack_size = value_pack_layout(self.agents)
        self.value_table = np.array([off["lstm.weight_ih_l0"][0] for off in self.offsets], dtype=np.int32)
        self._loaded = set()
        self._dev = None                # the device tensors, allocated once (a captured graph owns their addresses)
        self._out = {}                  # (T, N) -> dict of output tensors
        self._udev = None               # the epochs' gradient packs, Adam state and flags
        self._uout = {}                 # (T, N, groups) -> the epochs' workspace and outputs
        self._ulast = None

    # ------------------------------------------------------------------------------------------------ parameters
    def _index(self, agent_id):
        return packs.index(self.agent_ids, agent_id)

    def _device(self):
        if self._dev is None:
            import torch

            dev = torch.device("cuda", self.device)
            self._dev = {"pack": torch.zeros(self.pack_size, dtype=torch.float32, device=dev),
                         "vtable": torch.as_tensor(self.value_table, device=dev)}
        return self._dev

    def parameters(self, agent_id):
        """{key: float32 CUDA tensor} in torch's shapes; the tensors ALIAS the pack the kernel reads."""
        want = self.offsets[self._index(agent_id)]
        return packs.views(self._device()["pack"], want)

    def load_state_dict(self, agent_id, state_dict):
        """Copy a value network's tensors (the reference's keys; torch tensors or arrays) into the pack."""
        i = self._index(agent_id)
        packs.load(self.offsets[i], state_dict, lambda: self._device()["pack"])
        self._loaded.add(i)

    def bind(self, agent_id, value_module):
        """Copy the module's parameters into the pack and point every ``param.data`` at its view there."""
        packs.check_module(value_module, self.offsets[self._index(agent_id)])
        self.load_state_dict(agent_id, {k: v for k, v in value_module.state_dict().items()})
        return packs.repoint(value_module, self.parameters(agent_id))

    # ------------------------------------------------------------------------------------------------ the launch
    def evaluate(self, obs, actions, want_mu_std=False):
        """``obs`` [T + 1, N, n_obs] float32 and ``actions`` [T, N, n_actions] float32 or float64 (the actions whose log-probability is
        wanted: with delta actions the clamped delta, ``LstmActors.outputs["raw"]``), contiguous CUDA.  Returns ``{"values", "next_values":
        [T, N, n_agents], "old_log_probs": [T, N, n_actions]}`` and with ``want_mu_std`` also ``mu`` and ``std``, float32.  ``next_values``
        is the value LSTM run over ``obs[1:]`` from a zero state, as the reference runs it; it is not ``values[1:]``.  The outputs are
        allocated once per (T, N) and written again by the next call of that shape.  One launch on the current torch stream, no
        synchronisation: capturable."""
        import torch

        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[0] < 2 or obs.shape[1] < 1:
            raise ValueError("obs must be a torch tensor of shape [T + 1, N, n_obs] with T >= 1")
        T, N = int(obs.shape[0]) - 1, int(obs.shape[1])
        packs.check_tensor("obs", obs, self.device, (T + 1, N, self.n_obs))
        packs.check_tensor("actions", actions, self.device, (T, N, self.n_actions), (torch.float32, torch.float64))
        self._check_loaded()
        d = self._device()
        out = self._out.setdefault((T, N), {})
        dev = torch.device("cuda", self.device)
        if "old_log_probs" not in out:
            out["old_log_probs"] = torch.zeros(T, N, self.n_actions, dtype=torch.float32, device=dev)
            out["values"], out["next_values"] = (torch.zeros(T, N, self.n_agents, dtype=torch.float32, device=dev) for _ in range(2))
        if want_mu_std and "mu" not in out:
            out["mu"], out["std"] = (torch.zeros(T, N, self.n_actions, dtype=torch.float32, device=dev) for _ in range(2))
        ad = self.actors._device()
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(dev).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = lib.pedn_lstm_ppo_evaluate(p(obs), p(actions), p(ad["table"]), p(d["vtable"]), p(ad["pack"]), p(d["pack"]), p(out["values"]),
                                            p(out["next_values"]), p(out["old_log_probs"]), p(out["mu"]) if want_mu_std else None,
                                            p(out["std"]) if want_mu_std else None, T, N, self.n_obs, self.n_actions, self.n_agents, HIDDEN, 1,
                                            int(actions.dtype == torch.float64), self.actors.min_std, self.actors.max_std,
                                            C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise _launch_failed("pedn_lstm_ppo_evaluate", rc)
        keys = ("values", "next_values", "old_log_probs") + (("mu", "std") if want_mu_std else ())
        return {k: out[k] for k in keys}

    def _check_store(self, store):
        from .rollout import RolloutStore

        if not isinstance(store, RolloutStore):
            raise ValueError("store must be a RolloutStore")
        if store.rows is None:
            raise ValueError("call store.finish() first")
        if store.rows < 1:
            raise ValueError("the store holds no rows")
        if (store.n_obs, store.n_actions, store.n_agents) != (self.n_obs, self.n_actions, self.n_agents):
            raise ValueError("the store was not made for the env of these actors")

    def evaluate_store(self, store, actions=None, want_mu_std=False):
        """Behind ``store.finish()``: ``evaluate`` on the store's ``obs`` and by default its ``actions`` (float64; ``actions`` [rows,
        n_envs, n_actions] replaces them).  Returns the dict of ``evaluate``."""
        self._check_store(store)
        if not store.store_obs:
            raise ValueError("the store keeps no observations (rollout_store(store_obs=True))")
        v = store.views()
        return self.evaluate(v["obs"], v["actions"] if actions is None else actions, want_mu_std=want_mu_std)

    def compute_gae(self, store, values, next_values, gamma, lmbda):
        """(advantages, td_target) [rows, n_envs, n_agents] float32 from the store's rewards and done flags and the ``values`` /
        ``next_values`` of ``evaluate_store``: ``td_target = r + gamma * next_values * (1 - done)``, the RAW advantages (the reference's
        normalisation line stays a torch line of the caller).  One launch on the current torch stream."""
        from .rollout import gae

        self._check_store(store)
        v = store.views()
        shape = (store.rows, store.n_envs, self.n_agents)
        packs.check_tensor("values", values, self.device, shape)
        packs.check_tensor("next_values", next_values, self.device, shape)
        dones = v["done"].unsqueeze(-1).expand(*shape)
        return gae(v["rewards"], values, dones, gamma, lmbda, next_values=next_values)

    # ------------------------------------------------------------------------------------------------ the clipped-loss epochs
    def _check_loaded(self):
        self.actors._missing()
        missing = [self.agent_ids[i] for i in range(self.n_agents) if i not in self._loaded]
        if missing:
            raise ValueError(f"no value networks were loaded for {missing}: load_state_dict() or bind() first")

    def update_workspace_bytes(self, T, N, groups=None):
        """Bytes the epochs allocate for a rollout of ``T`` rows of ``N`` envs, once per (T, N, groups), with R = T * N:
        ``4 * (2 * n_agents * R * 384 + 4 * R * n_actions + min(ceil(R / 32), groups) * slab)``, slab = the actors' pack (rounded up to 4
        floats) + the value pack + 8 * n_agents floats.  The first term holds, per network, agent and row, the forward's h', c' and four
        gates, which back-propagation through time needs and overwrites with the gates' gradients: it grows with the rollout, about 2.2 GB
        per network and agent at 700 x 2048 rows -- it fits the card but is not small."""
        groups = self._groups(groups)
        if isinstance(T, bool) or isinstance(N, bool) or not isinstance(T, (int, np.integer)) or not isinstance(N, (int, np.integer)) or T < 1 or N < 1:
            raise ValueError("T and N must be positive integers")
        rows = int(T) * int(N)
        slab = -(-self.actors.pack_size // 4) * 4 + self.pack_size + 8 * self.n_agents
        return 4 * (2 * self.n_agents * rows * ROW_FLOATS + TAIL_PLANES * rows * self.n_actions + min(-(-rows // TILE), groups) * slab)

    def _epoch_launch(self, obs, actions, old_log_probs, advantages, td_target, args, groups, do_adam, want_tail=False):
        import torch

        actor_lr, critic_lr, clip_eps, max_grad_norm, kl_tolerance, b1, b2, eps = args
        groups = self._groups(groups)
        T, N = self._check_epoch_inputs(obs, actions, old_log_probs, advantages, td_target)
        d, ud, ad = self._device(), self._update_device(), self.actors._device()
        out = self._uout.get((T, N, groups))
        if out is None:
            dev = torch.device("cuda", self.device)
            rows = T * N
            slab = -(-self.actors.pack_size // 4) * 4 + self.pack_size + 8 * self.n_agents
            z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
            out = self._uout[(T, N, groups)] = {"ws": z(min(-(-rows // TILE), groups), slab), "act": z(2, self.n_agents, rows, ROW_FLOATS),
                                                "tail4": z(TAIL_PLANES, T, N, self.n_actions), "log_probs": z(T, N, self.n_actions),
                                                "values": z(T, N, self.n_agents)}
            assert 4 * sum(out[k].numel() for k in ("ws", "act", "tail4")) == self.update_workspace_bytes(T, N, groups)
        self._ulast = dict(out, tail=out["tail4"][:3] if want_tail else None)
        if ad["pack"].data_ptr() % 16:
            raise ValueError("the actors' pack is not 16-byte aligned")
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        ua, uv = ud["actor"], ud["value"]
        with torch.cuda.device(self.device):
            rc = lib.pedn_lstm_ppo_epoch_update(p(obs), p(actions), p(old_log_probs), p(advantages), p(td_target), p(ad["table"]), p(d["vtable"]),
                                                p(ad["pack"]), p(d["pack"]), p(ua["grads"]), p(uv["grads"]), p(ua["raw"]), p(uv["raw"]),
                                                p(ua["exp_avg"]), p(uv["exp_avg"]), p(ua["exp_avg_sq"]), p(uv["exp_avg_sq"]), p(out["ws"]),
                                                p(out["act"]), p(out["tail4"]), p(ud["parts"]), p(out["log_probs"]), p(out["values"]),
                                                p(ud["scalars"]), p(ud["adam"]), p(ud["flags"]), self.actors.pack_size, self.pack_size, T, N,
                                                self.n_obs, self.n_actions, self.n_agents, HIDDEN, 1, int(actions.dtype == torch.float64), groups,
                                                self.actors.min_std, self.actors.max_std, actor_lr, critic_lr, clip_eps, max_grad_norm,
                                                kl_tolerance, b1, b2, eps, 1 if do_adam else 0, C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise _launch_failed("pedn_lstm_ppo_epoch_update", rc)

    def update_store(self, store, old_log_probs, advantages, td_target, epochs=10, actor_lr=3e-4, critic_lr=6e-4, clip_eps=0.2, max_grad_norm=0.5,
                     kl_tolerance=0.01, betas=(0.9, 0.999), eps=1e-8, groups=None):
        """Behind ``store.finish()``, ``evaluate_store(store)``, ``compute_gae(...)`` and the caller's normalisation line: ``begin_update()``
        and ``epochs`` times ``epoch_update`` on the store's ``obs`` and ``actions``; every env's rows are one sequence from a zero state.
        On the current torch stream, which ``evaluate_store`` and ``compute_gae`` used too; no allocation after the first call of a shape
        (``update_workspace_bytes``), no synchronisation: capturable as one graph."""
        args = self._update_arguments(actor_lr, critic_lr, clip_eps, max_grad_norm, kl_tolerance, betas, eps)
        if isinstance(epochs, bool) or not isinstance(epochs, (int, np.integer)) or int(epochs) < 0:
            raise ValueError(f"epochs must be an integer and not negative, got {epochs!r}")
        groups = self._groups(groups)
        self._check_store(store)
        if not store.store_obs:
            raise ValueError("the store keeps no observations (rollout_store(store_obs=True))")
        v = store.views()
        self._check_epoch_inputs(v["obs"], v["actions"], old_log_probs, advantages, td_target)      # before begin_update()'s launch, and with epochs = 0
        self.begin_update()
        for _ in range(int(epochs)):
            self._epoch_launch(v["obs"], v["actions"], old_log_probs, advantages, td_target, args, groups, True)


def for_env(env, delta_actions=True, max_delta=2.5, min_std=1e-3, max_std=10.0, seed=0, hidden_size=HIDDEN, num_layers=1):
    """``LstmActors`` over the agents, slices, bounds and global env indices of a ``VecPedNetEnv``."""
    if not hasattr(env, "network") or not hasattr(env, "possible_agents") or hasattr(env, "groups"):
        raise ValueError("LSTM actors belong to one VecPedNetEnv (MultiScenarioVecEnv steps separate engines)")
    agents = [(env.obs_slices[a].start, env.obs_slices[a].stop - env.obs_slices[a].start,
               env.action_slices[a].start, env.action_slices[a].stop - env.action_slices[a].start) for a in env.possible_agents]
    return LstmActors(agents, env.action_low, env.action_high, env.n_envs, env.n_obs, env.n_actions, delta_actions=delta_actions,
                      max_delta=max_delta, min_std=min_std, max_std=max_std, seed=seed, replica_offset=env.network.replica_offset,
                      device=env.network.device, hidden_size=hidden_size, num_layers=num_layers, agent_ids=list(env.possible_agents))


def targets_for_env(env, actors):
    """``LstmPpoTargets`` over the LSTM actors of a ``VecPedNetEnv``."""
    if not hasattr(env, "network") or not hasattr(env, "possible_agents") or hasattr(env, "groups"):
        raise ValueError("LSTM PPO targets belong to one VecPedNetEnv (MultiScenarioVecEnv steps separate engines)")
    if isinstance(actors, LstmActors) and (actors.agent_ids != list(env.possible_agents) or actors.n_obs != env.n_obs or actors.n_actions != env.n_actions):
        raise ValueError("the actors were not made for this env (env.lstm_actors())")
    return LstmPpoTargets(actors)
