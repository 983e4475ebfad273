"""On-policy rollouts on the device: a transition store filled by one launch per policy step, and the reference's TD targets, GAE and
advantage normalisation (rl/agents/PPO_org.py:201-354,518-567; rl/rl_utils.py:1754-1773) for every (env, agent) trajectory at once
(pednstream_amd/csrc/pedn_rollout.hpp; the contract is DESIGN section 12, tests/rollout_model.py restates it in numpy).

    store = env.rollout_store()                       # capacity: the policy steps of an episode
    roll = env.capture(policy, on_step=lambda obs, rew: store.record(policy.last_actions, critic(obs)))
    env.reset(); store.begin()
    while not roll.step(): pass
    store.finish()
    adv, td_target = store.compute_gae(0.99, 0.95, normalize=True)

``gae`` is the functional form on plain tensors, ``compute_gae`` has the reference's signature.
"""
import ctypes as C

from . import engine as _engine

ARRAYS = {"actions": 0, "values": 1, "rewards": 2, "done": 3, "obs": 4, "td_target": 5, "advantages_raw": 6, "advantages_normalized": 7}


def _is(t, torch, dtype, shape):
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape))


class RolloutStore:
    """Device-resident store of up to ``capacity`` transitions of every env of a ``VecPedNetEnv`` (``env.rollout_store()``).  One fill
    is one episode, or a prefix of one: ``begin()`` after ``env.reset()``, ``record()`` after every policy step, ``finish()``."""

    def __init__(self, env, capacity=None, store_obs=True):
        if not hasattr(env, "network") or not hasattr(env, "possible_agents") or hasattr(env, "groups"):
            raise ValueError("a rollout store belongs to one VecPedNetEnv (MultiScenarioVecEnv steps separate engines)")
        if capacity is None:
            capacity = env.simulation_steps // env.action_gap
        if int(capacity) < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        self.env, self.capacity, self.store_obs = env, int(capacity), bool(store_obs)
        self.n_envs, self.n_agents, self.n_actions, self.n_obs = env.n_envs, len(env.possible_agents), env.n_actions, env.n_obs
        env.network._flush().rollout_configure(self.capacity, self.store_obs)
        self.rows, self.overflow = None, False
        self._begun = False
        self._normalized = None        # what the last compute_gae returned as advantages
        self._full = None

    # ------------------------------------------------------------------------------------------------ filling
    def _engine(self):
        if self.env._rollout_store is not self:
            raise ValueError("this store was replaced by a later rollout_store() call")
        return self.env.network.engine()

    def begin(self):
        """A new fill: the cursor back to row 0, ``obs[0]`` = the observation the env holds now (the reset observation)."""
        eng = self._engine()
        self.env.network._flush()
        eng.rollout_begin()
        self._begun, self.rows, self.overflow, self._normalized = True, None, False, None

    def record(self, actions, values=None):
        """Store the transition of the policy step that has just run: ``actions`` [n_envs, n_actions] float64 and ``values`` [n_envs,
        n_agents] float32 (V of the state the actions were decided in; None: zeros) are contiguous CUDA tensors; the rewards, the
        terminated flag and the next observation are taken from the engine.  One launch, no host synchronisation; inside ``on_step``
        of a captured rollout it is captured with the step."""
        import torch

        eng = self._engine()
        if not self._begun:
            raise ValueError("call begin() before record()")
        if not _is(actions, torch, torch.float64, (self.n_envs, self.n_actions)):
            raise ValueError(f"actions must be a contiguous float64 CUDA tensor of shape {(self.n_envs, self.n_actions)}")
        if values is not None and not _is(values, torch, torch.float32, (self.n_envs, self.n_agents)):
            raise ValueError(f"values must be a contiguous float32 CUDA tensor of shape {(self.n_envs, self.n_agents)}")
        env = self.env
        vp = values.data_ptr() if values is not None else 0
        dev = torch.device("cuda", env.network.device)
        cur = torch.cuda.current_stream(dev)
        if eng.rl_clocked():
            # a captured rollout (or between its replays): on the stream the step's launches are on; done comes from the device clock
            eng.rollout_record(actions.data_ptr(), vp, False, cur.cuda_stream)
        else:
            # eager stepping: on the engine's stream, chained to the caller's by events in both directions (the rows are ready when the
            # launch starts; whatever the caller does with the tensors next comes behind it)
            if env._ext_stream is None:
                env._ext_stream = torch.cuda.ExternalStream(eng.stream_ptr(), device=dev)
            env._ext_stream.wait_stream(cur)
            eng.rollout_record(actions.data_ptr(), vp, (env.sim_step - 1) >= env.simulation_steps, 0)
            cur.wait_stream(env._ext_stream)
        self.rows = None

    def finish(self, last_values=None):
        """Wait for the recorded rows; ``last_values`` [n_envs, n_agents] float32 (CUDA) is the bootstrap value V(s_T) of the state behind
        the last row (None: zeros -- irrelevant when the last row is terminated).  Returns the number of rows; ``overflow`` tells
        whether records beyond the capacity were dropped."""
        import torch

        eng = self._engine()
        if not self._begun:
            raise ValueError("call begin() before finish()")
        if last_values is not None:
            if not _is(last_values, torch, torch.float32, (self.n_envs, self.n_agents)):
                raise ValueError(f"last_values must be a contiguous float32 CUDA tensor of shape {(self.n_envs, self.n_agents)}")
            torch.cuda.current_stream(last_values.device).synchronize()
        self.rows, self.overflow = eng.rollout_finish(last_values.data_ptr() if last_values is not None else 0)
        return self.rows

    def compute_gae(self, gamma, lmbda, normalize=False):
        """(advantages, td_target) [rows, n_envs, n_agents] float32 views of the device arrays; ``normalize``: the reference's
        ``(adv - adv.mean()) / (adv.std() + 1e-8)`` per agent over all rows and envs (the raw advantages stay in ``views()``)."""
        eng = self._engine()
        if self.rows is None:
            raise ValueError("call finish() before compute_gae()")
        if normalize and self.rows * self.n_envs < 2:
            raise ValueError("advantage normalisation needs at least two entries per agent")
        eng.rollout_compute(gamma, lmbda, normalize)
        self._normalized = bool(normalize)
        v = self.views()
        return v["advantages"], v["td_target"]

    # ------------------------------------------------------------------------------------------------ reading
    def _arrays(self):
        import torch

        from .rl_env import _DeviceBuffer

        if self._full is None:
            eng = self._engine()
            dev = torch.device("cuda", self.env.network.device)
            c, n, a = self.capacity, self.n_envs, self.n_agents
            shapes = {"actions": ((c, n, self.n_actions), "<f8"), "values": ((c + 1, n, a), "<f4"), "rewards": ((c, n, a), "<f4"),
                      "done": ((c, n), "<f4"), "td_target": ((c, n, a), "<f4"), "advantages_raw": ((c, n, a), "<f4"),
                      "advantages_normalized": ((c, n, a), "<f4")}
            if self.store_obs:
                shapes["obs"] = ((c + 1, n, self.n_obs), "<f4")
            self._full = {k: torch.as_tensor(_DeviceBuffer(eng.rollout_device_ptr(ARRAYS[k]), shape, ty), device=dev)
                          for k, (shape, ty) in shapes.items()}
        return self._full

    def views(self):
        """Dict of torch tensors that ALIAS the device arrays (no host copy): ``actions`` f64 [rows, n_envs, n_actions], ``values``
        [rows + 1, n_envs, n_agents], ``rewards`` [rows, n_envs, n_agents], ``done`` [rows, n_envs], ``obs`` [rows + 1, n_envs, n_obs]
        (with ``store_obs``), and after ``compute_gae``: ``td_target``, ``advantages_raw`` and ``advantages`` (the normalised ones when
        they were asked for).  Before ``finish()`` the arrays have the full capacity."""
        self._engine()
        full = self._arrays()
        rows = self.capacity if self.rows is None else self.rows
        out = {k: full[k][:rows + (1 if k in ("values", "obs") else 0)] for k in ("actions", "values", "rewards", "done", "obs") if k in full}
        if self._normalized is not None and self.rows is not None:
            out["td_target"], out["advantages_raw"] = full["td_target"][:rows], full["advantages_raw"][:rows]
            out["advantages"] = full["advantages_normalized"][:rows] if self._normalized else out["advantages_raw"]
        return out

    def agent(self, aid):
        """The arrays of one agent, sliced the way ``split_obs`` slices an observation row."""
        env = self.env
        if aid not in env.action_slices:
            raise ValueError(f"Unknown agent: {aid}")
        i = env.possible_agents.index(aid)
        out = {}
        for k, t in self.views().items():
            if k == "actions":
                out[k] = t[..., env.action_slices[aid]]
            elif k == "obs":
                out[k] = t[..., env.obs_slices[aid]]
            elif k == "done":
                out[k] = t
            else:
                out[k] = t[..., i]
        return out

    def close(self):
        """Free the device arrays (views handed out before must not be used any more)."""
        if self.env._rollout_store is self:
            self.env.network._flush().rollout_free()
            self.env._rollout_store = None
        self._full = None


def _gae_call(rew, val, done, T, lanes, gamma, lmbda, td, adv, stream_ptr, nxt=None):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    lib, st = _engine.lib(), C.c_void_p(int(stream_ptr)) if stream_ptr else None
    if nxt is None:
        name, rc = "pedn_gae", lib.pedn_gae(p(rew), p(val), p(done), int(T), int(lanes), float(gamma), float(lmbda), p(td), p(adv), st)
    else:
        name, rc = "pedn_gae_next", lib.pedn_gae_next(p(rew), p(val), p(nxt), p(done), int(T), int(lanes), float(gamma), float(lmbda), p(td), p(adv), st)
    if rc != 0:
        raise (ValueError if rc == -1 else RuntimeError)(f"{name} failed ({rc}): {lib.pedn_last_error(None).decode()}")


def gae(rewards, values, dones, gamma, lmbda, next_values=None):
    """(advantages, td_target) of shape ``rewards.shape``: ``rewards`` and ``dones`` are float32 CUDA tensors [T, ...], ``values``
    [T + 1, ...] (row t = V(s_t), row T the bootstrap value); every trailing index is a trajectory of its own.  With ``next_values``
    [T, ...] (recurrent critics, whose next values are a run of their own: ``pednstream_amd.lstm``) row t's next value is
    ``next_values[t]`` and ``values`` is [T, ...].  One launch on the current torch stream, no host synchronisation."""
    import torch

    ok = lambda t: isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    if not (ok(rewards) and ok(values) and ok(dones)) or (next_values is not None and not ok(next_values)):
        raise ValueError("rewards, values and dones must be float32 CUDA tensors")
    if next_values is not None:
        if rewards.dim() < 1 or rewards.shape[0] < 1 or rewards[0].numel() < 1 or \
                not (tuple(dones.shape) == tuple(values.shape) == tuple(next_values.shape) == tuple(rewards.shape)):
            raise ValueError(f"expected rewards / dones / values / next_values [T, ...], got {tuple(rewards.shape)}, {tuple(dones.shape)}, "
                             f"{tuple(values.shape)}, {tuple(next_values.shape)}")
        if next_values.device != rewards.device:
            raise ValueError("rewards, values, next_values and dones must be on one device")
        next_values = next_values.contiguous()
    elif rewards.dim() < 1 or rewards.shape[0] < 1 or tuple(dones.shape) != tuple(rewards.shape) or \
            tuple(values.shape) != (rewards.shape[0] + 1,) + tuple(rewards.shape[1:]) or rewards[0].numel() < 1:
        raise ValueError(f"expected rewards / dones [T, ...] and values [T + 1, ...], got {tuple(rewards.shape)}, {tuple(dones.shape)}, "
                         f"{tuple(values.shape)}")
    if not (rewards.device == values.device == dones.device):
        raise ValueError("rewards, values and dones must be on one device")
    rewards, values, dones = rewards.contiguous(), values.contiguous(), dones.contiguous()
    T, lanes = rewards.shape[0], rewards[0].numel()
    with torch.cuda.device(rewards.device):
        adv, td = torch.empty_like(rewards), torch.empty_like(rewards)
        _gae_call(rewards, values, dones, T, lanes, gamma, lmbda, td, adv, torch.cuda.current_stream().cuda_stream, next_values)
    return adv, td


def compute_gae(gamma, lmbda, td_delta):
    """The reference's ``rl_utils.compute_gae(gamma, lmbda, td_delta)``: ``td_delta`` of shape (T, 1) or (T,) (CPU or CUDA) -> a float
    tensor of the same shape on the same device, computed by the device kernel (a CPU tensor makes the round trip)."""
    import torch

    if not isinstance(td_delta, torch.Tensor) or td_delta.dim() not in (1, 2) or (td_delta.dim() == 2 and td_delta.shape[1] != 1) \
            or td_delta.shape[0] < 1:
        raise ValueError("td_delta must be a tensor of shape (T, 1) or (T,)")
    if not td_delta.dtype.is_floating_point:
        raise ValueError("td_delta must be a floating-point tensor")
    dev = td_delta.device
    x = td_delta.detach().to(device="cuda" if dev.type != "cuda" else dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(x.device):
        adv = torch.empty_like(x)
        _gae_call(x, None, None, x.shape[0], 1, gamma, lmbda, None, adv, torch.cuda.current_stream().cuda_stream)
    return adv.to(dev)
