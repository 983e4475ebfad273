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
    ppo.update_store(store, old_log_probs, adv, td_target, epochs=10)   # the clipped-loss epochs, in place in both packs

``PpoTargets`` is the constructor on a ``StackedActors`` (no env).  The epochs run on the device too (``epoch_update``, ``update_store``:
both forwards, both backward passes, ``clip_grad_norm_``, both Adam steps and the KL early stop of every agent in three launches per epoch,
pednstream_amd/csrc/pedn_ppo_grad.hpp, DESIGN section 20, tests/ppo_update_model.py); torch modules bound to the packs see the steps and
can still run the epochs themselves (examples/ppo_update.py).
"""
import ctypes as C
import math

import numpy as np

from . import engine as _engine
from . import packs
from .policy import HIDDEN, StackedActors

TILE = 32                       # rows per workgroup of ppo_eval_kernel (PEDN_PPO_TILE) and per tile of ppograd_kernel: part of section 20's order of sums
DEFAULT_GROUPS = 512            # slabs of the epochs' workspace, workgroups per agent and network of ppograd_kernel: two per compute unit of an MI355X
SCALARS = ("actor_loss", "critic_loss", "approx_kl", "actor_norm", "value_norm", "actor_coef", "value_coef")      # per agent, pedn_ppo_epoch_update's order
ADAM_STATE_INIT = (0, 0, 0x3FF0000000000000, 0x3FF0000000000000)      # per agent: the step count, the ticket, the doubles beta1^0 and beta2^0


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


class EpochUpdates:
    """What the clipped-loss epochs of ``PpoTargets`` and of ``lstm.LstmPpoTargets`` share: the arguments' checks, the gradient packs, Adam
    state and flags on the device, the epoch calls and their outputs.  A subclass has ``actors`` (with ``pack_size`` and ``offsets``), its
    own ``pack_size`` / ``offsets``, ``_epoch_launch``, ``_check_loaded`` and the name of its ``_BEGIN`` export."""

    @staticmethod
    def _groups(groups):
        if groups is None:
            return DEFAULT_GROUPS
        if isinstance(groups, bool) or not isinstance(groups, (int, np.integer)) or not 1 <= int(groups) <= 65535:
            raise ValueError(f"groups must be an integer in 1 .. 65535, got {groups!r}")
        return int(groups)

    @staticmethod
    def _update_arguments(actor_lr, critic_lr, clip_eps, max_grad_norm, kl_tolerance, betas, eps):
        try:
            actor_lr, critic_lr, eps, (b1, b2) = float(actor_lr), float(critic_lr), float(eps), (float(b) for b in betas)
            clip_eps, max_grad_norm, kl_tolerance = float(clip_eps), float(max_grad_norm), float(kl_tolerance)
        except (TypeError, ValueError):
            raise ValueError("the learning rates, eps, clip_eps, max_grad_norm and kl_tolerance must be numbers and betas a pair of numbers") from None
        for name, lr in (("actor_lr", actor_lr), ("critic_lr", critic_lr)):
            if not (math.isfinite(lr) and lr >= 0.0):
                raise ValueError(f"{name} must be finite and not negative, got {lr}")
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"eps must be finite and not negative, got {eps}")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must be in [0, 1), got {(b1, b2)}")
        if not (math.isfinite(clip_eps) and clip_eps > 0.0):
            raise ValueError(f"clip_eps must be finite and positive, got {clip_eps}")
        if not (math.isfinite(max_grad_norm) and max_grad_norm > 0.0):
            raise ValueError(f"max_grad_norm must be finite and positive, got {max_grad_norm}")
        if math.isnan(kl_tolerance):
            raise ValueError("kl_tolerance must not be NaN")
        return actor_lr, critic_lr, clip_eps, max_grad_norm, kl_tolerance, b1, b2, eps

    def _update_device(self):
        if self._udev is None:
            import torch

            dev = torch.device("cuda", self.device)
            za = lambda: torch.zeros(-(-max(1, self.actors.pack_size) // 4) * 4, dtype=torch.float32, device=dev)
            zv = lambda: torch.zeros(self.pack_size, dtype=torch.float32, device=dev)
            self._udev = {"actor": {k: za() for k in ("grads", "raw", "exp_avg", "exp_avg_sq")},
                          "value": {k: zv() for k in ("grads", "raw", "exp_avg", "exp_avg_sq")},
                          "parts": torch.zeros(self.n_agents, 2, 16, dtype=torch.float64, device=dev),
                          "scalars": torch.zeros(len(SCALARS), self.n_agents, dtype=torch.float32, device=dev),
                          "adam": torch.tensor([ADAM_STATE_INIT] * self.n_agents, dtype=torch.int64, device=dev),
                          "flags": torch.zeros(self.n_agents, dtype=torch.int32, device=dev)}
        return self._udev

    def _check_epoch_inputs(self, obs, actions, old_log_probs, advantages, td_target):
        """(T, N) of an epoch's tensors, or ValueError: everything a launch reads, checked before any launch."""
        import torch

        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[0] < 2 or obs.shape[1] < 1:
            raise ValueError("obs must be a torch tensor of shape [T + 1, N, n_obs] with T >= 1")
        T, N = int(obs.shape[0]) - 1, int(obs.shape[1])
        packs.check_tensor("obs", obs, self.device, (T + 1, N, self.n_obs))
        packs.check_tensor("actions", actions, self.device, (T, N, self.n_actions), (torch.float32, torch.float64))
        packs.check_tensor("old_log_probs", old_log_probs, self.device, (T, N, self.n_actions))
        packs.check_tensor("advantages", advantages, self.device, (T, N, self.n_agents))
        packs.check_tensor("td_target", td_target, self.device, (T, N, self.n_agents))
        self._check_loaded()
        return T, N

    def epoch_update(self, obs, actions, old_log_probs, advantages, td_target, actor_lr=3e-4, critic_lr=6e-4, clip_eps=0.2, max_grad_norm=0.5,
                     kl_tolerance=0.01, betas=(0.9, 0.999), eps=1e-8, groups=None, want_tail=False):
        """ONE epoch of the reference's clipped-loss loop for every agent, in place in the actors' pack and the value pack: both
        forwards on every row of ``obs`` [T + 1, N, n_obs] / ``actions`` [T, N, n_actions] (``evaluate``'s inputs), the clipped surrogate
        against ``old_log_probs`` [T, N, n_actions] and ``advantages`` [T, N, n_agents], the MSE value loss against ``td_target`` [T, N,
        n_agents], both backward passes, ``clip_grad_norm_(max_grad_norm)`` of each network, one Adam step of each (``actor_lr``,
        ``critic_lr``) and the KL early stop: behind the step of an epoch whose ``approx_kl > 1.5 * kl_tolerance`` the agent's flag is set,
        and further epochs leave the agent untouched until ``begin_update()``.  ``groups``: how many slabs of the workspace share the
        tiles of 32 rows (part of the order of the sums; ``None``: ``DEFAULT_GROUPS``).  ``want_tail``: also write ``std``, ``d_mu`` and ``d_z``
        [T, N, n_actions] (the loss' gradients by mu and by the pre-softplus value; large for a whole rollout).  Three launches (the
        recurrent agents: five, over each env's whole sequence) on the current torch stream; no allocation after the first call of a (T, N,
        groups), no synchronisation: capturable."""
        args = self._update_arguments(actor_lr, critic_lr, clip_eps, max_grad_norm, kl_tolerance, betas, eps)
        self._epoch_launch(obs, actions, old_log_probs, advantages, td_target, args, groups, True, want_tail)

    def epoch_gradients(self, obs, actions, old_log_probs, advantages, td_target, clip_eps=0.2, max_grad_norm=0.5, groups=None, want_tail=False):
        """The launches of ``epoch_update`` with both Adam steps and the stop switched off: writes ``epoch_outputs``; no parameter, optimiser
        state, step count or flag changes (an agent whose flag is set is skipped all the same)."""
        args = self._update_arguments(0.0, 0.0, clip_eps, max_grad_norm, math.inf, (0.0, 0.0), 0.0)
        self._epoch_launch(obs, actions, old_log_probs, advantages, td_target, args, groups, False, want_tail)

    def begin_update(self):
        """Clear every agent's stop flag with a device-side write on the current torch stream (capturable): the start of an update's epochs."""
        import torch

        ud = self._update_device()
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = getattr(lib, self._BEGIN)(C.c_void_p(ud["flags"].data_ptr()), self.n_agents, C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"{self._BEGIN} failed ({rc}): {lib.pedn_last_error(None).decode()}")

    class _EpochOutputs:
        def __init__(self, owner, out):
            sc = owner._udev["scalars"]
            self.log_probs, self.values = out["log_probs"], out["values"]
            self.std, self.d_mu, self.d_z = out["tail"] if out["tail"] is not None else (None, None, None)
            for i, k in enumerate(SCALARS):
                setattr(self, k, sc[i])
            self.stop_flags, self._owner = owner._udev["flags"], owner

        def grads(self, agent_id, which, clipped=True):
            """{key: float32 CUDA tensor} in ``nn.Linear`` shapes, the keys of ``parameters()``: views of the gradient pack the caller
            reads, the clipped one (``clipped=False``: what ``clip_grad_norm_`` was given)."""
            o = self._owner
            i, name = o._index(agent_id), o._which(which)
            return packs.views(o._udev[name]["grads" if clipped else "raw"], (o.actors.offsets if name == "actor" else o.offsets)[i])

    @staticmethod
    def _which(which):
        if which not in ("actor", "value"):
            raise ValueError(f"which must be 'actor' or 'value', got {which!r}")
        return which

    @property
    def epoch_outputs(self):
        """What the last ``epoch_update`` / ``epoch_gradients`` wrote, float32: ``log_probs`` [T, N, n_actions], ``values`` [T, N,
        n_agents]; per agent ``actor_loss``, ``critic_loss``, ``approx_kl``, ``actor_norm``, ``value_norm``, ``actor_coef``,
        ``value_coef``; ``stop_flags`` int32 [n_agents]; ``grads(agent_id, "actor" | "value")``; and, when the call asked for them (``want_tail``), ``std``,
        ``d_mu``, ``d_z`` [T, N, n_actions] (``None`` otherwise)."""
        if self._ulast is None:
            raise ValueError("epoch_update() has not run")
        return self._EpochOutputs(self, self._ulast)

    def adam_state(self, agent_id, which):
        """({key: exp_avg}, {key: exp_avg_sq}) of an agent's actor or value network: views of the optimiser's packs."""
        i, name = self._index(agent_id), self._which(which)
        ud, off = self._update_device()[name], (self.actors.offsets if name == "actor" else self.offsets)[i]
        return packs.views(ud["exp_avg"], off), packs.views(ud["exp_avg_sq"], off)

    def adam_steps(self):
        """[n_agents] how many Adam steps each agent's two networks have made (the device counters; waits for the device): agents stop
        independently."""
        return [int(v) for v in self._update_device()["adam"][:, 0].tolist()]

    def reset_adam(self):
        """Zero both networks' exp_avg and exp_avg_sq and every agent's step count."""
        import torch

        ud = self._update_device()
        for name in ("actor", "value"):
            ud[name]["exp_avg"].zero_()
            ud[name]["exp_avg_sq"].zero_()
        ud["adam"].copy_(torch.tensor([ADAM_STATE_INIT] * self.n_agents, dtype=torch.int64))


class PpoTargets(EpochUpdates):
    """``actors``: a ``StackedActors`` of kind "ppo"; the agent table, ``min_std`` / ``max_std``, the device and the stack size are its.
    The actors' pack is read in place; the value networks live in a pack of their own."""

    _BEGIN = "pedn_ppo_begin_update"

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

    # ------------------------------------------------------------------------------------------------ the clipped-loss epochs
    def update_workspace_shape(self, rows, groups=None):
        """(slabs, floats per slab) of the epochs' workspace for ``rows`` = T * N rows: ``min(ceil(rows / 32), groups)`` slabs, each the
        actors' pack (rounded up to 4 floats), the value pack and per agent three partial sums in double (8 floats).  It does not grow with ``rows`` beyond
        ``groups`` tiles."""
        groups = self._groups(groups)
        if int(rows) < 1:
            raise ValueError("the number of rows must be positive")
        return min(-(-int(rows) // TILE), groups), -(-self.actors.pack_size // 4) * 4 + self.pack_size + 8 * self.n_agents

    def _epoch_launch(self, obs, actions, old_log_probs, advantages, td_target, args, groups, do_adam, want_tail=False):
        import torch

        actor_lr, critic_lr, clip_eps, max_grad_norm, kl_tolerance, b1, b2, eps = args
        groups = self._groups(groups)
        T, N = self._check_epoch_inputs(obs, actions, old_log_probs, advantages, td_target)
        d, ud, ad = self._device(), self._update_device(), self.actors._device()
        out = self._uout.get((T, N, groups))
        if out is None:
            dev = torch.device("cuda", self.device)
            out = self._uout[(T, N, groups)] = {"ws": torch.zeros(*self.update_workspace_shape(T * N, groups), dtype=torch.float32, device=dev),
                                                "log_probs": torch.zeros(T, N, self.n_actions, dtype=torch.float32, device=dev),
                                                "values": torch.zeros(T, N, self.n_agents, dtype=torch.float32, device=dev)}
        if want_tail and "tail" not in out:
            out["tail"] = torch.zeros(3, T, N, self.n_actions, dtype=torch.float32, device=torch.device("cuda", self.device))
        self._ulast = dict(out, tail=out["tail"] if want_tail else None)
        if ad["pack"].data_ptr() % 16:
            raise ValueError("the actors' pack is not 16-byte aligned")
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        ua, uv = ud["actor"], ud["value"]
        with torch.cuda.device(self.device):
            rc = lib.pedn_ppo_epoch_update(p(obs), p(actions), p(old_log_probs), p(advantages), p(td_target), p(ad["table"]), p(d["vtable"]),
                                           p(ad["pack"]), p(d["pack"]), p(ua["grads"]), p(uv["grads"]), p(ua["raw"]), p(uv["raw"]),
                                           p(ua["exp_avg"]), p(uv["exp_avg"]), p(ua["exp_avg_sq"]), p(uv["exp_avg_sq"]), p(out["ws"]),
                                           p(ud["parts"]), p(out["log_probs"]), p(out["values"]), p(out["tail"]) if want_tail else None, p(ud["scalars"]), p(ud["adam"]), p(ud["flags"]),
                                           self.actors.pack_size, self.pack_size, T, N, self.stack_size, self.n_obs, self.n_actions,
                                           self.n_agents, HIDDEN, int(actions.dtype == torch.float64), groups, self.actors.min_std,
                                           self.actors.max_std, actor_lr, critic_lr, clip_eps, max_grad_norm, kl_tolerance, b1, b2, eps,
                                           1 if do_adam else 0, C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"pedn_ppo_epoch_update failed ({rc}): {lib.pedn_last_error(None).decode()}")

    def _check_loaded(self):
        missing = [self.agent_ids[i] for i in range(self.n_agents) if i not in self.actors._loaded]
        if missing:
            raise ValueError(f"no actor parameters were loaded for {missing}: StackedActors.load_state_dict() or bind() first")
        missing = [self.agent_ids[i] for i in range(self.n_agents) if i not in self._loaded]
        if missing:
            raise ValueError(f"no value networks were loaded for {missing}: load_state_dict() or bind() first")

    def update_store(self, store, old_log_probs, advantages, td_target, epochs=10, actor_lr=3e-4, critic_lr=6e-4, clip_eps=0.2, max_grad_norm=0.5,
                     kl_tolerance=0.01, betas=(0.9, 0.999), eps=1e-8, groups=None):
        """Behind ``store.finish()``, ``evaluate_store(store)`` and ``store.compute_gae(..., normalize=True)``: ``begin_update()`` and
        ``epochs`` times ``epoch_update`` on the store's ``obs`` and ``actions``.  Capturable as one graph."""
        from .rollout import RolloutStore

        args = self._update_arguments(actor_lr, critic_lr, clip_eps, max_grad_norm, kl_tolerance, betas, eps)
        if isinstance(epochs, bool) or not isinstance(epochs, (int, np.integer)) or int(epochs) < 0:
            raise ValueError(f"epochs must be an integer and not negative, got {epochs!r}")
        groups = self._groups(groups)
        if not isinstance(store, RolloutStore):
            raise ValueError("store must be a RolloutStore")
        if not store.store_obs:
            raise ValueError("the store keeps no observations (rollout_store(store_obs=True))")
        if store.rows is None:
            raise ValueError("call store.finish() before update_store()")
        if store.rows < 1:
            raise ValueError("the store holds no rows")
        if (store.n_obs, store.n_actions, store.n_agents) != (self.n_obs, self.n_actions, self.n_agents):
            raise ValueError("the store was not made for the env of these actors")
        v = store.views()
        self._check_epoch_inputs(v["obs"], v["actions"], old_log_probs, advantages, td_target)      # before begin_update()'s launch, and with epochs = 0
        # compute_gae ran on the engine's stream: the caller's waits (on the device) for the advantages and targets written there
        import torch

        env = store.env
        dev = torch.device("cuda", env.network.device)
        if not torch.cuda.is_current_stream_capturing():
            if env._ext_stream is None:
                env._ext_stream = torch.cuda.ExternalStream(store._engine().stream_ptr(), device=dev)
            torch.cuda.current_stream(dev).wait_stream(env._ext_stream)
        self.begin_update()
        for _ in range(int(epochs)):
            self._epoch_launch(v["obs"], v["actions"], old_log_probs, advantages, td_target, args, groups, True)

def for_env(env, actors):
    """``PpoTargets`` over the stacked actors of a ``VecPedNetEnv``."""
    if not hasattr(env, "network") or not hasattr(env, "possible_agents") or hasattr(env, "groups"):
        raise ValueError("PPO targets belong to one VecPedNetEnv (MultiScenarioVecEnv steps separate engines)")
    if isinstance(actors, StackedActors) and (actors.agent_ids != list(env.possible_agents) or actors.n_obs != env.n_obs or actors.n_actions != env.n_actions):
        raise ValueError("the actors were not made for this env (env.stacked_actors('ppo', stack_size))")
    return PpoTargets(actors)
