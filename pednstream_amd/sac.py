"""The gradient-free half of the reference's ``SACAgent.update`` on the device, for every agent at once: the TD targets of a whole-row
minibatch in ONE launch (``calc_target``, rl/agents/SAC.py:296-312, with both target critics ``QValueNetContinuous`` :109-125) and the
Polyak update of every target critic in ONE launch (``soft_update`` :314-318).  pednstream_amd/csrc/pedn_sac.hpp; the contract is DESIGN
section 15, tests/sac_target_model.py restates it in numpy.

    buf = env.replay_store(capacity, stack_size=5)
    actors = env.stacked_actors(kind="sac", stack_size=5)
    sac = env.sac_targets(actors)
    for aid in env.possible_agents:
        sac.bind(aid, critic_1[aid], critic_2[aid], target_1[aid], target_2[aid], log_alpha=log_alpha[aid])
    s, a, r, ns, d, idx = buf.sample(256)
    td = sac.td_target(r, ns, d)                  # [256, n_agents], detached by construction
    sac.critic_update(s, a.float(), td)           # or the losses and optimiser steps in torch, on the bound modules
    sac.actor_update(s)
    sac.soft_update()

``SacTargets`` is the constructor on a ``StackedActors`` (no env).

The critic step of the gradient half runs on the device too (pednstream_amd/csrc/pedn_critic.hpp; the contract is DESIGN section 18,
tests/sac_critic_model.py restates it in numpy): ``sac.critic_update(s, critic_actions, td)`` between ``td_target`` and ``soft_update`` computes
q1, q2, both MSE losses, their gradients and one Adam step of every online critic in two launches.

So does the actor half (pednstream_amd/csrc/pedn_actor_grad.hpp; the contract is DESIGN section 19, tests/sac_actor_model.py restates it
in numpy): ``sac.actor_update(s)`` behind ``critic_update`` computes the actor loss through both stepped online critics, its gradient, one
Adam step of every actor in the ``StackedActors`` pack, and the temperature loss with one Adam step of every ``log_alpha``, in two
launches.  sample -> td_target -> critic_update -> actor_update -> soft_update is a whole SAC update with no torch module in it.
"""
import ctypes as C
import math

import numpy as np

from . import engine as _engine
from . import packs
from .policy import HIDDEN, StackedActors

WHICH = ("critic_1", "critic_2", "target_critic_1", "target_critic_2")
ACTION_OUTPUTS = ("mu", "std", "eps", "logp", "next_actions")
AGENT_OUTPUTS = ("entropy", "q1", "q2", "td_target")
ACTOR_ACTION_OUTPUTS = ("mu", "std", "eps", "logp", "new_actions", "z", "t", "d_mu", "d_z")      # z: the pre-softplus value; t = tanh(mu + std * eps); d_*: the loss' gradients
ACTOR_AGENT_OUTPUTS = ("entropy", "q1", "q2")
TILE = 8                        # rows per workgroup of sac_target_kernel (PEDN_SAC_TILE)
CRITIC_TILE = 32                # rows per workgroup of critic_grad_kernel (PEDN_GRAD_TILE): part of section 18's order of sums
ADAM_STATE_INIT = (0, 0, 0x3FF0000000000000, 0x3FF0000000000000)      # the step count, the ticket, the doubles beta1^0 and beta2^0


def critic_shapes(obs_w, act_w, stack_size, hidden_size=HIDDEN):
    """[(state_dict key, shape)] of one critic in the order of the pack."""
    h = int(hidden_size)
    return [("encoder.fc1.weight", (h, int(stack_size) * int(obs_w))), ("encoder.fc1.bias", (h,)), ("encoder.fc2.weight", (h, h)),
            ("encoder.fc2.bias", (h,)), ("fc.weight", (h, h + int(act_w) + 1)), ("fc.bias", (h,)), ("fc_out.weight", (1, h)), ("fc_out.bias", (1,))]


def critic_pack_layout(agents, stack_size, hidden_size=HIDDEN):
    """(offsets, total): offsets[i][c] = {key: (offset in floats, shape)} of critic c + 1 of agent i = (obs0, obs_w, act0, act_w); per
    agent critic 1 then critic 2, every critic on a multiple of 4 floats; total is a multiple of 4 (the padding is zero)."""
    flat, total = packs.layout([critic_shapes(obs_w, act_w, stack_size, hidden_size) for (_, obs_w, _, act_w) in agents for _c in range(2)])
    return [flat[2 * i:2 * i + 2] for i in range(len(agents))], total


def make_critic_module(obs_w, act_w, stack_size):
    """A torch module with the reference critic's layers, parameter names and forward (``forward(s [B, S, obs_w], a [B, act_w]) ->
    [B, 1]``), for training beside the kernel: ``SacTargets.bind`` makes its parameters views of a pack."""
    import torch
    from torch import nn

    class Critic(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder, self.fc, self.fc_out = packs.make_encoder(obs_w, stack_size), nn.Linear(HIDDEN + int(act_w) + 1, HIDDEN), nn.Linear(HIDDEN, 1)

        def forward(self, s, a):
            zs = self.encoder(s.transpose(1, 2).flatten(1))               # input f * S + s is s[b, s, f]
            gate_widths = s[:, -1, -1].unsqueeze(1)                       # the newest frame's last column
            return self.fc_out(self.fc(torch.cat([zs, a, gate_widths], dim=1)))      # (no ReLU behind fc, as in the reference)

    return Critic()


class SacTargets:
    """``actors``: a ``StackedActors`` of kind "sac"; the agent table, ``max_delta``, the device and the stack size are its.  The actors'
    pack is read in place; the critics live in two packs of one layout, ``online`` and ``target``."""

    def __init__(self, actors, gamma=0.99, tau=0.005, seed=0):
        if not isinstance(actors, StackedActors):
            raise ValueError("actors must be a StackedActors")
        if actors.kind != "sac":
            raise ValueError(f"SAC targets need actors of kind 'sac', got {actors.kind!r}")
        gamma, tau = float(gamma), float(tau)
        if not math.isfinite(gamma):
            raise ValueError(f"gamma must be finite, got {gamma}")
        if not 0.0 <= tau <= 1.0:
            raise ValueError(f"tau must be in [0, 1], got {tau}")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("the seed must fit 64 bits")
        self.actors, self.gamma, self.tau, self.seed = actors, gamma, tau, int(seed)
        self.agents, self.agent_ids, self.device = actors.agents, actors.agent_ids, actors.device
        self.stack_size, self.n_obs, self.n_actions, self.max_delta = actors.stack_size, actors.n_obs, actors.n_actions, actors.max_delta
        self.n_agents = len(self.agents)
        self.offsets, self.pack_size = critic_pack_layout(self.agents, self.stack_size)
        self.critic_table = np.array([[pair[0]["encoder.fc1.weight"][0], pair[1]["encoder.fc1.weight"][0]] for pair in self.offsets], dtype=np.int32)
        self._loaded = set()            # (agent index, which)
        self._dev = None                # the device tensors, allocated once (a captured graph owns their addresses)
        self._out = {}                  # batch size -> (out_actions [5, B, n_actions], out_agents [4, B, n_agents])
        self._last = None
        self._cdev = None               # the critic step's device tensors, allocated by its first use
        self._cout = {}                 # batch size -> (workspace [tiles, stride], q [2, B, n_agents])
        self._clast = None
        self._adev = None               # the actor step's device tensors, allocated by its first use
        self._aout = {}                 # batch size -> (workspace [tiles, stride], actions' outputs [5, B, n_actions], agents' outputs [3, B, n_agents])
        self._alast = None
        self._tent = None               # the target entropies on the device, as the host last set them

    # ------------------------------------------------------------------------------------------------ parameters
    def _index(self, agent_id):
        return packs.index(self.agent_ids, agent_id)

    @staticmethod
    def _which(which):
        if which not in WHICH:
            raise ValueError(f"which must be one of {WHICH}, got {which!r}")
        return ("target" if which.startswith("target_") else "online"), int(which[-1]) - 1

    def _device(self):
        if self._dev is None:
            import torch

            dev = torch.device("cuda", self.device)
            self._dev = {"online": torch.zeros(self.pack_size, dtype=torch.float32, device=dev),
                         "target": torch.zeros(self.pack_size, dtype=torch.float32, device=dev),
                         "ctable": torch.as_tensor(self.critic_table, device=dev),
                         "log_alpha": torch.full((self.n_agents,), math.log(0.01), dtype=torch.float32, device=dev),
                         "state": torch.zeros(2, dtype=torch.int64, device=dev)}
        return self._dev

    def parameters(self, agent_id, which):
        """{key: float32 CUDA tensor} in ``nn.Linear`` shapes; the tensors ALIAS the pack the kernels read and write."""
        i = self._index(agent_id)
        pack_name, c = self._which(which)
        return packs.views(self._device()[pack_name], self.offsets[i][c])

    def load_state_dict(self, agent_id, which, state_dict):
        """Copy a critic's tensors (the reference's keys, ``nn.Linear`` layout; torch tensors or arrays) into its pack."""
        i = self._index(agent_id)
        pack_name, c = self._which(which)
        packs.load(self.offsets[i][c], state_dict, lambda: self._device()[pack_name])
        self._loaded.add((i, which))

    @property
    def log_alpha(self):
        """float32 [n_agents] CUDA tensor the kernel reads (default log 0.01)."""
        return self._device()["log_alpha"]

    def bind(self, agent_id, critic_1, critic_2, target_critic_1, target_critic_2, log_alpha=None):
        """Copy the four modules' parameters into the packs and point every ``param.data`` at its view there: an optimiser that steps
        the online critics updates what ``soft_update`` reads, and ``soft_update`` updates the target modules, with no copy.  A
        ``log_alpha`` leaf tensor's value is copied into its element of ``self.log_alpha`` and its ``.data`` becomes a view of it."""
        import torch

        i = self._index(agent_id)
        if log_alpha is not None and (not isinstance(log_alpha, torch.Tensor) or log_alpha.numel() != 1):
            raise ValueError("log_alpha must be a torch tensor of one element")
        modules = dict(zip(WHICH, (critic_1, critic_2, target_critic_1, target_critic_2)))
        for which, m in modules.items():
            packs.check_module(m, self.offsets[i][0], f"{which}: ")
        for which, m in modules.items():
            self.load_state_dict(agent_id, which, {k: v for k, v in m.state_dict().items()})
            packs.repoint(m, self.parameters(agent_id, which))
        if log_alpha is not None:
            view = self.log_alpha[i:i + 1].view(log_alpha.shape)
            with torch.no_grad():
                view.copy_(log_alpha.detach().to(torch.float32))
            log_alpha.data = view
        return modules

    # ------------------------------------------------------------------------------------------------ the two launches
    def td_target(self, rewards, next_states, dones, noise=None):
        """``td_target`` float32 [B, n_agents] (one tensor per batch size, written again by the next call of that size) for a whole-row
        minibatch as ``ReplayStore.sample(B)`` hands it out: ``rewards`` [B, n_agents], ``next_states`` [B, stack_size, n_obs], ``dones``
        [B], float32 contiguous CUDA.  ``noise`` [B, n_actions] float32: use it as eps in place of a draw.  One launch on the current
        torch stream; no allocation after the first call of a batch size, no synchronisation: capturable.  A draw advances ``draws()``."""
        import torch

        if not isinstance(dones, torch.Tensor) or dones.dim() != 1 or dones.shape[0] < 1:
            raise ValueError("dones must be a torch tensor of shape [B]")
        B = int(dones.shape[0])
        packs.check_tensor("dones", dones, self.device, (B,))
        packs.check_tensor("rewards", rewards, self.device, (B, self.n_agents))
        packs.check_tensor("next_states", next_states, self.device, (B, self.stack_size, self.n_obs))
        if noise is not None:
            packs.check_tensor("noise", noise, self.device, (B, self.n_actions))
        missing = [self.agent_ids[i] for i in range(self.n_agents) if i not in self.actors._loaded]
        if missing:
            raise ValueError(f"no actor parameters were loaded for {missing}: StackedActors.load_state_dict() or bind() first")
        missing = [(self.agent_ids[i], w) for i in range(self.n_agents) for w in WHICH[2:] if (i, w) not in self._loaded]
        if missing:
            raise ValueError(f"no critics were loaded for {missing}: load_state_dict() or bind() first")
        d = self._device()
        out = self._out.get(B)
        if out is None:
            dev = torch.device("cuda", self.device)
            out = self._out[B] = (torch.zeros(len(ACTION_OUTPUTS), B, self.n_actions, dtype=torch.float32, device=dev),
                                  torch.zeros(len(AGENT_OUTPUTS), B, self.n_agents, dtype=torch.float32, device=dev))
        self._last = out
        ad = self.actors._device()
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = lib.pedn_sac_td_target(p(next_states), p(rewards), p(dones), p(ad["table"]), p(d["ctable"]), p(ad["pack"]), p(d["target"]),
                                        p(d["log_alpha"]), p(noise) if noise is not None else None, p(out[0]), p(out[1]), p(d["state"]),
                                        B, self.stack_size, self.n_obs, self.n_actions, self.n_agents, HIDDEN, self.max_delta, self.gamma,
                                        self.seed, C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"pedn_sac_td_target failed ({rc}): {lib.pedn_last_error(None).decode()}")
        return out[1][3]

    @property
    def outputs(self):
        """What the last ``td_target`` wrote, float32: ``mu``, ``std``, ``eps``, ``logp``, ``next_actions`` [B, n_actions] and ``entropy``,
        ``q1``, ``q2``, ``td_target`` [B, n_agents]."""
        if self._last is None:
            raise ValueError("td_target() has not run")
        out = {k: self._last[0][i] for i, k in enumerate(ACTION_OUTPUTS)}
        out.update({k: self._last[1][i] for i, k in enumerate(AGENT_OUTPUTS)})
        return out

    def soft_update(self):
        """target = target * (1 - tau) + online * tau over every target critic: one launch on the current torch stream, capturable."""
        import torch

        missing = [(self.agent_ids[i], w) for i in range(self.n_agents) for w in WHICH if (i, w) not in self._loaded]
        if missing:
            raise ValueError(f"no critics were loaded for {missing}: load_state_dict() or bind() first")
        d = self._device()
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = lib.pedn_sac_soft_update(C.c_void_p(d["target"].data_ptr()), C.c_void_p(d["online"].data_ptr()), self.pack_size, self.tau,
                                          C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"pedn_sac_soft_update failed ({rc}): {lib.pedn_last_error(None).decode()}")

    # ------------------------------------------------------------------------------------------------ the critic step
    def critic_workspace_shape(self, batch):
        """(tiles, floats per tile) of the workspace of a batch size: per tile of ``CRITIC_TILE`` rows a partial gradient in the layout of
        the pack and, behind it, the [n_agents][2] partial sums of squares, rounded up to 4 floats."""
        if int(batch) < 1:
            raise ValueError("the batch size must be positive")
        return -(-int(batch) // CRITIC_TILE), self.pack_size + -(-2 * self.n_agents // 4) * 4

    def _critic_device(self):
        if self._cdev is None:
            import torch

            dev = torch.device("cuda", self.device)
            z = lambda: torch.zeros(self.pack_size, dtype=torch.float32, device=dev)
            self._cdev = {"grads": z(), "exp_avg": z(), "exp_avg_sq": z(), "losses": torch.zeros(self.n_agents, 2, dtype=torch.float32, device=dev),
                          "adam": torch.tensor(ADAM_STATE_INIT, dtype=torch.int64, device=dev)}
        return self._cdev

    @staticmethod
    def _adam_arguments(lr, betas, eps):
        try:
            lr, eps, (b1, b2) = float(lr), float(eps), (float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError("lr and eps must be numbers and betas a pair of numbers") from None
        if not (math.isfinite(lr) and lr >= 0.0):
            raise ValueError(f"lr must be finite and not negative, got {lr}")
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"eps must be finite and not negative, got {eps}")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must be in [0, 1), got {(b1, b2)}")
        return lr, b1, b2, eps

    def _critic_launch(self, states, actions, td_target, lr, betas, eps, do_adam):
        import torch

        lr, b1, b2, eps = self._adam_arguments(lr, betas, eps)
        if not isinstance(td_target, torch.Tensor) or td_target.dim() != 2 or td_target.shape[0] < 1:
            raise ValueError("td_target must be a torch tensor of shape [B, n_agents]")
        B = int(td_target.shape[0])
        packs.check_tensor("td_target", td_target, self.device, (B, self.n_agents))
        packs.check_tensor("states", states, self.device, (B, self.stack_size, self.n_obs))
        packs.check_tensor("actions", actions, self.device, (B, self.n_actions))
        missing = [(self.agent_ids[i], w) for i in range(self.n_agents) for w in WHICH[:2] if (i, w) not in self._loaded]
        if missing:
            raise ValueError(f"no critics were loaded for {missing}: load_state_dict() or bind() first")
        d, cd = self._device(), self._critic_device()
        out = self._cout.get(B)
        if out is None:
            dev = torch.device("cuda", self.device)
            out = self._cout[B] = (torch.zeros(*self.critic_workspace_shape(B), dtype=torch.float32, device=dev),
                                   torch.zeros(2, B, self.n_agents, dtype=torch.float32, device=dev))
        self._clast = out
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = lib.pedn_sac_critic_update(p(states), p(actions), p(td_target), p(self.actors._device()["table"]), p(d["ctable"]), p(d["online"]),
                                            p(cd["grads"]), p(cd["exp_avg"]), p(cd["exp_avg_sq"]), p(out[0]), p(out[1]), p(cd["losses"]), p(cd["adam"]),
                                            self.pack_size, B, self.stack_size, self.n_obs, self.n_actions, self.n_agents, HIDDEN, lr, b1, b2, eps,
                                            1 if do_adam else 0, C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"pedn_sac_critic_update failed ({rc}): {lib.pedn_last_error(None).decode()}")

    def critic_update(self, states, actions, td_target, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        """The critic half of the reference's ``update`` for every agent: q1 and q2 of ``states`` [B, stack_size, n_obs] and ``actions``
        [B, n_actions] (what the critics see: the stored actions, the delta when ``delta_actions`` is on), the two losses
        mean((q - td_target)^2) against ``td_target`` [B, n_agents], their gradients and one Adam step (torch's defaults otherwise) of
        every online critic, in place in the ``online`` pack.  float32 contiguous CUDA tensors.  Two launches on the current torch stream;
        no allocation after the first call of a batch size, no synchronisation: capturable.  The step count lives on the device."""
        self._critic_launch(states, actions, td_target, lr, betas, eps, True)

    def critic_gradients(self, states, actions, td_target):
        """The launches of ``critic_update`` with the Adam step switched off: writes the gradients, the losses and q
        (``critic_outputs``); no parameter and no optimiser state changes."""
        self._critic_launch(states, actions, td_target, 0.0, (0.0, 0.0), 0.0, False)

    class _CriticOutputs:
        def __init__(self, owner, q):
            self.q1, self.q2, self.losses, self._owner = q[0], q[1], owner._cdev["losses"], owner

        def grads(self, agent_id, which):
            """{key: float32 CUDA tensor} in ``nn.Linear`` shapes, the keys of ``parameters()``: views of the gradient pack."""
            o = self._owner
            pack_name, c = o._which(which)
            if pack_name != "online":
                raise ValueError("only the online critics have gradients")
            return packs.views(o._cdev["grads"], o.offsets[o._index(agent_id)][c])

    @property
    def critic_outputs(self):
        """What the last ``critic_update`` / ``critic_gradients`` wrote, float32: ``q1``, ``q2`` [B, n_agents], ``losses`` [n_agents, 2]
        and ``grads(agent_id, which)``."""
        if self._clast is None:
            raise ValueError("critic_update() has not run")
        return self._CriticOutputs(self, self._clast[1])

    def adam_state(self, agent_id, which):
        """({key: exp_avg}, {key: exp_avg_sq}) of an online critic: views of the optimiser's two packs."""
        i = self._index(agent_id)
        pack_name, c = self._which(which)
        if pack_name != "online":
            raise ValueError("only the online critics have an optimiser")
        cd = self._critic_device()
        return packs.views(cd["exp_avg"], self.offsets[i][c]), packs.views(cd["exp_avg_sq"], self.offsets[i][c])

    def adam_steps(self):
        """How many Adam steps ``critic_update`` has made (the device counter; waits for the device)."""
        return int(self._critic_device()["adam"][0].item())

    def reset_adam(self):
        """Zero exp_avg, exp_avg_sq and the step count."""
        import torch

        cd = self._critic_device()
        cd["exp_avg"].zero_()
        cd["exp_avg_sq"].zero_()
        cd["adam"].copy_(torch.tensor(ADAM_STATE_INIT, dtype=torch.int64))

    def draws(self):
        """How many launches have drawn noise (the device counter; waits for the device)."""
        return int(self._device()["state"][0].item())

    # ------------------------------------------------------------------------------------------------ the actor and temperature step
    def actor_workspace_shape(self, batch):
        """(tiles, floats per tile) of the actor step's workspace of a batch size: per tile of ``CRITIC_TILE`` rows a partial gradient in
        the layout of the actors' pack, rounded up to 4 floats, and behind it the [n_agents][2] partial sums of ``-alpha * entropy -
        min_q`` and of ``entropy - target_entropy``, rounded up to 4 floats."""
        if int(batch) < 1:
            raise ValueError("the batch size must be positive")
        return -(-int(batch) // CRITIC_TILE), -(-self.actors.pack_size // 4) * 4 + -(-2 * self.n_agents // 4) * 4

    def _actor_device(self):
        if self._adev is None:
            import torch

            dev = torch.device("cuda", self.device)
            z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
            n = max(1, self.actors.pack_size)
            self._adev = {"grads": z(n), "exp_avg": z(n), "exp_avg_sq": z(n), "alpha_moments": z(2, self.n_agents), "scalars": z(3, self.n_agents),
                          "target_entropy": z(self.n_agents), "adam": torch.tensor(ADAM_STATE_INIT, dtype=torch.int64, device=dev),
                          "state": torch.zeros(2, dtype=torch.int64, device=dev)}
            self._tent = None
        return self._adev

    def _target_entropy(self, target_entropy):
        """float32 [n_agents] on the host: ``None`` is -act_w of each agent (what the reference's trainer passes), a number serves all."""
        if target_entropy is None:
            return np.array([-float(aw) for (_, _, _, aw) in self.agents], dtype=np.float32)
        try:
            te = np.asarray(target_entropy, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("target_entropy must be a number or one number per agent") from None
        if te.ndim == 0:
            te = np.full(self.n_agents, float(te))
        if te.shape != (self.n_agents,):
            raise ValueError(f"target_entropy must be a number or {self.n_agents} numbers, got shape {te.shape}")
        if not np.isfinite(te).all():
            raise ValueError(f"target_entropy must be finite, got {te.tolist()}")
        return te.astype(np.float32)

    def _actor_launch(self, states, noise, actor_lr, alpha_lr, target_entropy, betas, eps, do_adam):
        import torch

        actor_lr, b1, b2, eps = self._adam_arguments(actor_lr, betas, eps)
        alpha_lr = self._adam_arguments(alpha_lr, betas, eps)[0]
        te = self._target_entropy(target_entropy)
        if not isinstance(states, torch.Tensor) or states.dim() != 3 or states.shape[0] < 1:
            raise ValueError("states must be a torch tensor of shape [B, stack_size, n_obs]")
        B = int(states.shape[0])
        packs.check_tensor("states", states, self.device, (B, self.stack_size, self.n_obs))
        if noise is not None:
            packs.check_tensor("noise", noise, self.device, (B, self.n_actions))
        missing = [self.agent_ids[i] for i in range(self.n_agents) if i not in self.actors._loaded]
        if missing:
            raise ValueError(f"no actor parameters were loaded for {missing}: StackedActors.load_state_dict() or bind() first")
        missing = [(self.agent_ids[i], w) for i in range(self.n_agents) for w in WHICH[:2] if (i, w) not in self._loaded]
        if missing:
            raise ValueError(f"no critics were loaded for {missing}: load_state_dict() or bind() first")
        d, ad, pd = self._device(), self._actor_device(), self.actors._device()
        if self._tent is None or not np.array_equal(self._tent, te):      # (a copy outside any capture: the values are the caller's constants)
            ad["target_entropy"].copy_(torch.as_tensor(te))
            self._tent = te
        out = self._aout.get(B)
        if out is None:
            dev = torch.device("cuda", self.device)
            out = self._aout[B] = (torch.zeros(*self.actor_workspace_shape(B), dtype=torch.float32, device=dev),
                                   torch.zeros(len(ACTOR_ACTION_OUTPUTS), B, self.n_actions, dtype=torch.float32, device=dev),
                                   torch.zeros(len(ACTOR_AGENT_OUTPUTS), B, self.n_agents, dtype=torch.float32, device=dev))
        self._alast = out
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        lib = _engine.lib()
        with torch.cuda.device(self.device):
            rc = lib.pedn_sac_actor_update(p(states), p(noise) if noise is not None else None, p(pd["table"]), p(d["ctable"]), p(pd["pack"]),
                                           p(d["online"]), p(d["log_alpha"]), p(ad["target_entropy"]), p(ad["grads"]), p(ad["exp_avg"]),
                                           p(ad["exp_avg_sq"]), p(ad["alpha_moments"]), p(out[0]), p(out[1]), p(out[2]), p(ad["scalars"]),
                                           p(ad["adam"]), p(ad["state"]), self.actors.pack_size, B, self.stack_size, self.n_obs, self.n_actions,
                                           self.n_agents, HIDDEN, self.max_delta, actor_lr, alpha_lr, b1, b2, eps, self.seed,
                                           1 if do_adam else 0, C.c_void_p(int(stream)) if stream else None)
        if rc != 0:
            raise (ValueError if rc == -1 else RuntimeError)(f"pedn_sac_actor_update failed ({rc}): {lib.pedn_last_error(None).decode()}")

    def actor_update(self, states, noise=None, actor_lr=3e-4, alpha_lr=3e-4, target_entropy=None, betas=(0.9, 0.999), eps=1e-8):
        """The actor half of the reference's ``update`` for every agent, behind ``critic_update``: the actor's forward on ``states``
        [B, stack_size, n_obs], the squashed sample and its log-probability, both ONLINE critics on (states, new_actions), the loss
        mean(-alpha * entropy - min(q1, q2)), its gradient through the critics' action inputs and the actor, one Adam step (torch's
        defaults otherwise) of every actor in place in the ``StackedActors`` pack, and the temperature's loss mean((entropy -
        target_entropy) * alpha) with one Adam step of every ``log_alpha`` element.  The critics are read, not written.  ``noise``
        [B, n_actions] float32 replaces the draw; ``target_entropy``: a number, one per agent, or ``None`` for -act_w.  Two launches on
        the current torch stream; no allocation after the first call of a batch size, no synchronisation: capturable (a new
        ``target_entropy`` is copied to the device by the call that brings it, so pass the same one while capturing and replaying).  The
        step count and the draw counter live on the device."""
        self._actor_launch(states, noise, actor_lr, alpha_lr, target_entropy, betas, eps, True)

    def actor_gradients(self, states, noise=None, target_entropy=None):
        """The launches of ``actor_update`` with both Adam steps switched off: writes the gradients, the losses and the forward's
        outputs (``actor_outputs``); no parameter and no optimiser state changes (a draw advances ``actor_draws()``)."""
        self._actor_launch(states, noise, 0.0, 0.0, target_entropy, (0.0, 0.0), 0.0, False)

    class _ActorOutputs:
        def __init__(self, owner, out):
            for i, k in enumerate(ACTOR_ACTION_OUTPUTS):
                setattr(self, k, out[1][i])
            for i, k in enumerate(ACTOR_AGENT_OUTPUTS):
                setattr(self, k, out[2][i])
            sc = owner._adev["scalars"]
            self.actor_loss, self.alpha_loss, self.alpha_grad, self._owner = sc[0], sc[1], sc[2], owner

        def grads(self, agent_id):
            """{key: float32 CUDA tensor} in ``nn.Linear`` shapes, the keys of ``StackedActors.parameters()``: views of the gradient pack."""
            o = self._owner
            return packs.views(o._adev["grads"], o.actors.offsets[o._index(agent_id)])

    @property
    def actor_outputs(self):
        """What the last ``actor_update`` / ``actor_gradients`` wrote, float32: ``mu``, ``std``, ``eps``, ``logp``, ``new_actions``
        (and ``z``, ``t``, ``d_mu``, ``d_z``: the pre-softplus value, tanh(mu + std * eps) and the loss' gradients by mu and z) [B, n_actions]; ``entropy``, ``q1``, ``q2`` [B, n_agents]; ``actor_loss``, ``alpha_loss``, ``alpha_grad`` [n_agents]; and
        ``grads(agent_id)``."""
        if self._alast is None:
            raise ValueError("actor_update() has not run")
        return self._ActorOutputs(self, self._alast)

    def actor_adam_state(self, agent_id):
        """({key: exp_avg}, {key: exp_avg_sq}) of an actor: views of the optimiser's two packs, with the agent's ``log_alpha`` moments
        (one element each) under the key ``"log_alpha"``."""
        i = self._index(agent_id)
        ad = self._actor_device()
        m, v = packs.views(ad["exp_avg"], self.actors.offsets[i]), packs.views(ad["exp_avg_sq"], self.actors.offsets[i])
        m["log_alpha"], v["log_alpha"] = ad["alpha_moments"][0, i:i + 1], ad["alpha_moments"][1, i:i + 1]
        return m, v

    def actor_adam_steps(self):
        """How many Adam steps ``actor_update`` has made (the device counter; waits for the device)."""
        return int(self._actor_device()["adam"][0].item())

    def reset_actor_adam(self):
        """Zero the actors' and the temperatures' exp_avg, exp_avg_sq and the step count."""
        import torch

        ad = self._actor_device()
        for k in ("exp_avg", "exp_avg_sq", "alpha_moments"):
            ad[k].zero_()
        ad["adam"].copy_(torch.tensor(ADAM_STATE_INIT, dtype=torch.int64))

    def actor_draws(self):
        """How many ``actor_update`` / ``actor_gradients`` launches have drawn noise (the device counter; waits for the device)."""
        return int(self._actor_device()["state"][0].item())


def for_env(env, actors, gamma=0.99, tau=0.005, seed=0):
    """``SacTargets`` over the stacked actors of a ``VecPedNetEnv``."""
    if not hasattr(env, "network") or not hasattr(env, "possible_agents") or hasattr(env, "groups"):
        raise ValueError("SAC targets belong to one VecPedNetEnv (MultiScenarioVecEnv steps separate engines)")
    if isinstance(actors, StackedActors) and (actors.agent_ids != list(env.possible_agents) or actors.n_obs != env.n_obs or actors.n_actions != env.n_actions):
        raise ValueError("the actors were not made for this env (env.stacked_actors('sac', stack_size))")
    return SacTargets(actors, gamma=gamma, tau=tau, seed=seed)
