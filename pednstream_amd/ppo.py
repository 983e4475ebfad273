"""The gradient-free half of the reference's ``PPOAgent.update`` on the device, for every agent, env and row of a rollout in ONE launch:
the value critics on every state (``StackedValueNetwork``, rl/agents/PPO_org.py:175-197; ``current_values`` and ``next_values`` of
:543-561 are rows t and t + 1 of one array) and ``old_log_probs = Normal(*actor(states)).log_prob(actions)`` (:569-577) with the stacked
actors that acted.  The stacks are put together on the fly from the observations the rollout store keeps once.
pednstream_amd/csrc/pedn_ppo.hpp; the contract is DESIGN section 16, tests/ppo_eval_model.py restates it in numpy.

    buf = env.replay_store(capacity, stack_size=5)                  # the acting stacks
    actors = env.stacked_actors(kind="ppo", stack_size=5)
    store = env.rollout_store()
    ppo = env.ppo_targets(actors)
    for aid in env.possible_agents:
        actors.bind(aid, actor[aid]); ppo.bind(aid, value_net[aid])
    roll = env.capture(lambda obs: actors.act(buf.stacked_obs()),
                       on_step=lambda obs, rew: (buf.push(actors.actions), store.record(actors.outputs["raw"].double(), None)))
    ...                                                             # the episode
    store.finish()
    old_log_probs = ppo.evaluate_store(store)                       # values[0 .. rows] are in the store now
    adv, td_target = store.compute_gae(0.99, 0.95, normalize=True)
    ...                                                             # the clipped-loss epochs in torch, on the bound modules

``PpoTargets`` is the constructor on a ``StackedActors`` (no env).  Backward passes, the optimisers and the KL early stop stay in torch.
"""
import ctypes as C

import numpy as np

from . import engine as _engine
from . import packs
from .policy import HIDDEN, StackedActors

TILE = 32                       # rows per workgroup of ppo_eval_kernel (PEDN_PPO_TILE)


def value_tensor_shapes(obs_w, stack_size, hidden_size=HIDDEN):
    """[(state_dict key, shape)] of one value network in the order of the pack."""
    h = int(hidden_size)
    return [("encoder.fc1.weight", (h, int(stack_size) * int(obs_w))), ("encoder.fc1.bias", (h,)), ("encoder.fc2.weight", (h, h)),
            ("encoder.fc2.bias", (h,)), ("fc.weight", (h, h)), ("fc.bias", (h,)), ("value_head.weight", (1, h)), ("value_head.bias", (1,))]


def value_pack_layout(agents, stack_size, hidden_size=HIDDEN):
    """(offsets, total): offsets[i] = {key: (offset in floats, shape)} of the value network of agent i = (obs0, obs_w, act0, act_w), one
    agent behind the other, every agent on a multiple of 4 floats; total is a multiple of 4 (the padding is zero)."""
    return packs.layout([value_tensor_shapes(obs_w, stack_size, hidden_size) for (_, obs_w, _, _) in agents])


def make_value_module(obs_w, stack_size):
    """A torch module with the reference value network's layers, parameter names and forward (``forward(x [B, S, obs_w]) -> [B, 1]``), for
    training beside the kernel: ``PpoTargets.bind`` makes its parameters views of the pack."""
    import torch
    from torch import nn

    class Value(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder, self.fc, self.value_head = packs.make_encoder(obs_w, stack_size), nn.Linear(HIDDEN, HIDDEN), nn.Linear(HIDDEN, 1)

        def forward(self, x):
            zs = self.encoder(x.transpose(1, 2).flatten(1))               # input f * S + s is x[b, s, f]
            return self.value_head(torch.relu(self.fc(zs)))               # (no LayerNorm, as in the reference)

    return Value()


class PpoTargets:
    """``actors``: a ``StackedActors`` of kind "ppo"; the agent table, ``min_std`` / ``max_std``, the device and the stack size are its.
    The actors' pack is read in place; the value networks live in a pack of their own."""

    def __init__(self, actors):
        if not isinstance(actors, StackedActors):
            raise ValueError("actors must be a StackedActors")
        if actors.kind != "ppo":
            raise ValueError(f"PPO targets need actors of kind 'ppo', got {actors.kind!r}")
        self.actors = actors
        self.agents, self.agent_ids, self.device = actors.agents, actors.agent_ids, actors.device
        self.stack_size, self.n_obs, self.n_actions = actors.stack_size, actors.n_obs, actors.n_actions
        self.n_agents = len(self.agents)
        self.offsets, self.pack_size = value_pack_layout(self.agents, self.stack_size)
        self.value_table = np.array([off["encoder.fc1.weight"][0] for off in self.offsets], dtype=np.int32)
        self._loaded = set()
        self._dev = None                # the device tensors, allocated once (a captured graph owns their addresses)
        self._out = {}                  # (T, N) -> dict of output tensors

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
        """{key: float32 CUDA tensor} in ``nn.Linear`` shapes; the tensors ALIAS the pack the kernel reads."""
        want = self.offsets[self._index(agent_id)]
        return packs.views(self._device()["pack"], want)

    def load_state_dict(self, agent_id, state_dict):
        """Copy a value network's tensors (the reference's keys, ``nn.Linear`` layout; torch tensors or arrays) into the pack."""
        i = self._index(agent_id)
        packs.load(self.offsets[i], state_dict, lambda: self._device()["pack"])
        self._loaded.add(i)

    def bind(self, agent_id, value_module):
        """Copy the module's parameters into the pack and point every ``param.data`` at its view there: an optimiser that steps the
        module updates what the next launch reads, with no copy per update."""
        packs.check_module(value_module, self.offsets[self._index(agent_id)])
        self.load_state_dict(agent_id, {k: v for k, v in value_module.state_dict().items()})
        return packs.repoint(value_module, self.parameters(agent_id))

    # ------------------------------------------------------------------------------------------------ the launch
    def evaluate(self, obs, actions, values_out=None, want_mu_std=False):
        """``obs`` [T + 1, N, n_obs] float32 and ``actions`` [T, N, n_actions] float32 or float64 (the actions whose log-probability is
        wanted: with delta actions the clamped delta, ``StackedActors.outputs["raw"]``), contiguous CUDA.  Returns ``{"values": [T + 1, N,
        n_agents], "old_log_probs": [T, N, n_actions]}`` and with ``want_mu_std`` also ``mu`` and ``std`` [T, N, n_actions], float32;
        ``values[t + 1]`` is the reference's ``next_values[t]``.  ``values_out``: write the values there instead (a contiguous float32
        tensor of that shape, the store's own array for one).  The outputs are allocated once per (T, N) and written again by the next
        call of that shape.  One launch on the current torch stream, no synchronisation: capturable."""
        import torch

        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[0] < 2 or obs.shape[1] < 1:
            raise ValueError("obs must be a torch tensor of shape [T + 1, N, n_obs] with T >= 1")
        T, N = int(obs.shape[0]) - 1, int(obs.shape[1])
        packs.check_tensor("obs", obs, self.device, (T + 1, N, self.n_obs))
        packs.check_tensor("actions", actions, self.device, (T, N, self.n_actions), (torch.float32, torch.float64))
        if values_out is not None:
            packs.check_tensor("values_out", values_out, self.device, (T + 1, N, self.n_agents))
        missing = [self.agent_ids[i] for i in range(self.n_agents) if i not in self.actors._loaded]
        if missing:
            raise ValueError(f"no actor parameters were loaded for {missing}: StackedActors.load_state_dict() or bind() first")
        missing = [self.agent_ids[i] for i in range(self.n_agents) if i not in self._loaded]
        if missing:
            raise ValueError(f"no value networks were loaded for {missing}: load_state_dict() or bind() first")
        d = self._device()
        out = self._out.setdefault((T, N), {})
        dev = torch.device("cuda", self.device)
        if "old_log_probs" not in out:
            out["old_log_probs"] = torch.zeros(T, N, self.n_actions, dtype=torch.float32, device=dev)
        if values_out is None and "values" not in out:
            out["values"] = torch.zeros(T + 1, N, self.n_agents, dtype=torch.float32, device=dev)
        if want_mu_std and "mu" not in out:
            out["mu"], out["std"] = (torch.zeros(T, N, self.n_actions, dtype=torch.float32, device=dev) for _ in range(2))
        values = values_out if values_out is not None else out["values"]
        ad = self.actors._device()
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(dev).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = lib.pedn_ppo_evaluate(p(obs), p(actions), p(ad["table"]), p(d["vtable"]), p(ad["pack"]), p(d["pack"]), p(values),
                                       p(out["old_log_probs"]), p(out["mu"]) if want_mu_std else None, p(out["std"]) if want_mu_std else None,
                                       T, N, self.stack_size, self.n_obs, self.n_actions, self.n_agents, HIDDEN,
                                       int(actions.dtype == torch.float64), self.actors.min_std, self.actors.max_std,
                                       C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"pedn_ppo_evaluate failed ({rc}): {lib.pedn_last_error(None).decode()}")
        res = {"values": values, "old_log_probs": out["old_log_probs"]}
        if want_mu_std:
            res["mu"], res["std"] = out["mu"], out["std"]
        return res

    def evaluate_store(self, store, actions=None, want_mu_std=False):
        """Behind ``store.finish()``: evaluate the rows of the fill from the store's ``obs`` and by default its ``actions`` (float64;
        ``actions`` [rows, n_envs, n_actions] replaces them), write ``values[0 .. rows]`` into the store's own ``values`` array -- a
        following ``store.compute_gae(gamma, lmbda, normalize=True)`` yields the reference's ``td_target`` and advantages with no critic
        call per step -- and return ``old_log_probs`` [rows, n_envs, n_actions] (with ``want_mu_std`` the whole dict of ``evaluate``)."""
        from .rollout import RolloutStore

        if not isinstance(store, RolloutStore):
            raise ValueError("store must be a RolloutStore")
        if not store.store_obs:
            raise ValueError("the store keeps no observations (rollout_store(store_obs=True))")
        if store.rows is None:
            raise ValueError("call store.finish() before evaluate_store()")
        if store.rows < 1:
            raise ValueError("the store holds no rows")
        if (store.n_obs, store.n_actions, store.n_agents) != (self.n_obs, self.n_actions, self.n_agents):
            raise ValueError("the store was not made for the env of these actors")
        v = store.views()
        res = self.evaluate(v["obs"], v["actions"] if actions is None else actions, values_out=v["values"], want_mu_std=want_mu_std)
        # compute_gae launches on the engine's stream: it waits (on the device) for the values written on the caller's
        import torch

        env = store.env
        dev = torch.device("cuda", env.network.device)
        if not torch.cuda.is_current_stream_capturing():
            if env._ext_stream is None:
                env._ext_stream = torch.cuda.ExternalStream(store._engine().stream_ptr(), device=dev)
            env._ext_stream.wait_stream(torch.cuda.current_stream(dev))
        return res if want_mu_std else res["old_log_probs"]


def for_env(env, actors):
    """``PpoTargets`` over the stacked actors of a ``VecPedNetEnv``."""
    if not hasattr(env, "network") or not hasattr(env, "possible_agents") or hasattr(env, "groups"):
        raise ValueError("PPO targets belong to one VecPedNetEnv (MultiScenarioVecEnv steps separate engines)")
    if isinstance(actors, StackedActors) and (actors.agent_ids != list(env.possible_agents) or actors.n_obs != env.n_obs or actors.n_actions != env.n_actions):
        raise ValueError("the actors were not made for this env (env.stacked_actors('ppo', stack_size))")
    return PpoTargets(actors)
