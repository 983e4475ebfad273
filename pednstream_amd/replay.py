"""Off-policy replay on the device: a ring of transitions of the whole env batch that keeps every observation once, a stacked
observation for the policy, and minibatches of stacked transitions gathered by one launch (the counterpart of rl/rl_utils.py:37-50
ReplayBuffer under rl/agents/SAC.py:127-225; pednstream_amd/csrc/pedn_replay.hpp; the contract is DESIGN section 13, tests/replay_model.py
restates it in numpy).

    buf = env.replay_store(capacity, stack_size=4, seed=0)        # capacity in rows: one row = one policy step of all envs
    roll = env.capture(lambda obs: policy(buf.stacked_obs()), on_step=lambda obs, rew: buf.push(policy.last_actions))
    env.reset(); buf.begin()
    while not roll.step():
        for aid in env.possible_agents:
            s, a, r, ns, d, idx = buf.sample(64, agent=aid)
"""
ARRAYS = {"frames": 0, "actions": 1, "rewards": 2, "done": 3, "first": 4, "step_serial": 5, "stacked": 6, "state": 7}


def ring_slots(capacity, stack_size, episode_steps):
    """R: room for the newest ``capacity`` STEP rows, the RESET rows between them, the frames under the oldest one's stack, and the
    row being written."""
    return capacity + stack_size + -(-capacity // episode_steps) + 1


class ReplayStore:
    """Device-resident replay buffer of a ``VecPedNetEnv`` (``env.replay_store()``): ``begin()`` after every ``env.reset()``, ``push()``
    after every policy step, ``sample()`` whenever a minibatch is wanted."""

    def __init__(self, env, capacity, stack_size=4, seed=0):
        if not hasattr(env, "network") or not hasattr(env, "possible_agents") or hasattr(env, "groups"):
            raise ValueError("a replay store belongs to one VecPedNetEnv (MultiScenarioVecEnv steps separate engines)")
        if int(capacity) < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        if int(stack_size) < 1:
            raise ValueError(f"stack_size must be positive, got {stack_size}")
        self.env, self.capacity, self.stack_size, self.seed = env, int(capacity), int(stack_size), int(seed)
        self.n_envs, self.n_agents, self.n_actions, self.n_obs = env.n_envs, len(env.possible_agents), env.n_actions, env.n_obs
        self.episode_steps = max(1, env.simulation_steps // env.action_gap)
        self.ring_slots = ring_slots(self.capacity, self.stack_size, self.episode_steps)
        env.network._flush().replay_configure(self.capacity, self.stack_size, self.episode_steps, self.seed)
        self._begun = False
        self._pushes = 0               # push launches issued (a captured one counts once): 0 = the host knows the store is empty
        self._full = None
        self._out = {}                 # (batch_size, agent) -> the output tensors of sample()

    def _engine(self):
        if self.env._replay_store is not self:
            raise ValueError("this store was closed or replaced by a later replay_store() call")
        return self.env.network.engine()

    # ------------------------------------------------------------------------------------------------ filling
    def begin(self):
        """A new episode: a RESET row with the observation the env holds now; ``stacked_obs()`` becomes ``stack_size`` copies of it."""
        eng = self._engine()
        self.env.network._flush()
        eng.replay_begin()
        self.env._ordered_behind_engine()          # the policy reads stacked_obs() on the caller's stream
        self._begun = True

    def push(self, actions):
        """Store the transition of the policy step that has just run: ``actions`` [n_envs, n_actions] is a contiguous float64 CUDA
        tensor; the rewards, the terminated flag and the next observation are taken from the engine.  One launch, no host
        synchronisation; inside ``on_step`` of a captured rollout it is captured with the step."""
        import torch

        eng = self._engine()
        if not self._begun:
            raise ValueError("call begin() before push()")
        if not _is(actions, torch, torch.float64, (self.n_envs, self.n_actions), self.env.network.device):
            raise ValueError(f"actions must be a contiguous float64 CUDA tensor of shape {(self.n_envs, self.n_actions)}")
        env = self.env
        dev = torch.device("cuda", env.network.device)
        cur = torch.cuda.current_stream(dev)
        if eng.rl_clocked():
            # a captured rollout (or between its replays): on the stream the step's launches are on; done comes from the device clock
            eng.replay_push(actions.data_ptr(), False, cur.cuda_stream)
        else:
            # eager stepping: on the engine's stream, chained to the caller's by events in both directions
            if env._ext_stream is None:
                env._ext_stream = torch.cuda.ExternalStream(eng.stream_ptr(), device=dev)
            env._ext_stream.wait_stream(cur)
            eng.replay_push(actions.data_ptr(), (env.sim_step - 1) >= env.simulation_steps, 0)
            cur.wait_stream(env._ext_stream)
        self._pushes += 1

    def stacked_obs(self):
        """[n_envs, stack_size, n_obs] float32, oldest frame first: the state the next action is decided in.  It ALIASES the device
        buffer that every ``begin`` / ``push`` launch rewrites, so a captured policy reads it in place."""
        return self._arrays()["stacked"]

    # ------------------------------------------------------------------------------------------------ sampling
    def _columns(self, agent):
        env = self.env
        if agent is None:
            return (0, self.n_obs), (0, self.n_actions), (0, self.n_agents)
        if agent not in env.action_slices:
            raise ValueError(f"Unknown agent: {agent}")
        o, a = env.obs_slices[agent], env.action_slices[agent]
        return (o.start, o.stop - o.start), (a.start, a.stop - a.start), (env.possible_agents.index(agent), 1)

    def sample(self, batch_size=None, agent=None, indices=None):
        """``(states, actions, rewards, next_states, dones, idx)`` of ``batch_size`` transitions drawn with replacement on the device,
        or of the given ``indices`` ([B, 2] int64 CUDA: (serial, env) pairs, e.g. the ``idx`` of an earlier call -- every agent's
        columns of ONE draw).  ``agent=None``: whole rows, states [B, stack_size, n_obs], actions [B, n_actions] float64, rewards
        [B, n_agents], dones [B]; ``agent=aid``: that agent's columns in the shapes of ``SACAgent.update``, (B, stack_size, obs_dim),
        (B, act_dim), (B,), (B,).  One launch on the current stream, no host synchronisation, capturable.  The tensors are allocated
        once per (batch_size, agent) and written again by the next such call."""
        import torch

        eng = self._engine()
        dev = torch.device("cuda", self.env.network.device)
        if indices is not None:
            if not (isinstance(indices, torch.Tensor) and indices.is_cuda and indices.device == dev and indices.dtype == torch.int64
                    and indices.is_contiguous() and indices.dim() == 2 and indices.shape[1] == 2 and indices.shape[0] >= 1):
                raise ValueError("indices must be a contiguous int64 CUDA tensor of shape [B, 2]: (serial, env) pairs")
            if batch_size is not None and int(batch_size) != indices.shape[0]:
                raise ValueError(f"batch_size {batch_size} does not match {indices.shape[0]} indices")
            batch_size = indices.shape[0]
        if batch_size is None or int(batch_size) < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        B = int(batch_size)
        obs, act, rew = self._columns(agent)
        if self._pushes == 0:
            raise ValueError("the store is empty: nothing has been pushed")
        out = self._out.get((B, agent))
        if out is None:
            f32 = dict(dtype=torch.float32, device=dev)
            out = self._out[(B, agent)] = (torch.zeros(B, self.stack_size, obs[1], **f32), torch.zeros(B, act[1], dtype=torch.float64, device=dev),
                                           torch.zeros((B, rew[1]) if agent is None else (B,), **f32), torch.zeros(B, self.stack_size, obs[1], **f32),
                                           torch.zeros(B, **f32), torch.zeros(B, 2, dtype=torch.int64, device=dev))
        s, a, r, ns, d, idx = out
        eng.replay_sample(B, indices.data_ptr() if indices is not None else 0, obs, act, rew,
                          (s.data_ptr(), a.data_ptr(), r.data_ptr(), ns.data_ptr(), d.data_ptr(), 0 if indices is not None else idx.data_ptr()),
                          torch.cuda.current_stream(dev).cuda_stream)
        return s, a, r, ns, d, (indices if indices is not None else idx)

    # ------------------------------------------------------------------------------------------------ reading
    def state(self):
        """Waits for the device: dict of ``head`` (the next serial), ``steps`` (STEP rows so far), ``size_rows``, ``first`` (the RESET
        serial of the running episode), ``draws``.  A sample that was not sampleable since the last look raises RuntimeError here."""
        st = self._engine().replay_state()
        if st.pop("error"):
            raise RuntimeError("a sample asked for a transition that is not in the replay store (an empty store, an evicted or RESET "
                               "serial, or an env out of range): its output rows were left as they were")
        return st

    def size_rows(self):
        """Sampleable rows (device state; waits for the device)."""
        return self.state()["size_rows"]

    def size(self):
        """Sampleable transitions: ``size_rows() * n_envs``."""
        return self.size_rows() * self.n_envs

    def _arrays(self):
        import torch

        from .rl_env import _DeviceBuffer

        if self._full is None:
            eng = self._engine()
            dev = torch.device("cuda", self.env.network.device)
            R, n = self.ring_slots, self.n_envs
            shapes = {"frames": ((R, n, self.n_obs), "<f4"), "actions": ((R, n, self.n_actions), "<f8"), "rewards": ((R, n, self.n_agents), "<f4"),
                      "done": ((R,), "<f4"), "first": ((R,), "<i8"), "step_serial": ((self.capacity,), "<i8"),
                      "stacked": ((n, self.stack_size, self.n_obs), "<f4")}
            self._full = {k: torch.as_tensor(_DeviceBuffer(eng.replay_device_ptr(ARRAYS[k]), shape, ty), device=dev)
                          for k, (shape, ty) in shapes.items()}
        return self._full

    def views(self):
        """Dict of torch tensors that ALIAS the ring (no host copy): ``frames`` [R, n_envs, n_obs], ``actions`` f64 [R, n_envs,
        n_actions], ``rewards`` [R, n_envs, n_agents], ``done`` [R], ``first`` i64 [R], ``step_serial`` i64 [capacity], ``stacked``."""
        return dict(self._arrays())

    @property
    def nbytes(self):
        """Device bytes of the ring and its tables."""
        R, n, f = self.ring_slots, self.n_envs, 4
        return R * n * (self.n_obs * f + self.n_actions * 8 + self.n_agents * f) + R * (f + 8) + self.capacity * 8 + \
            n * self.stack_size * self.n_obs * f + 64

    def close(self):
        """Free the device arrays (views and samples handed out before must not be used any more); reports a pending sample error."""
        if self.env._replay_store is self:
            try:
                self.state()
            finally:
                self.env.network._flush().replay_free()
                self.env._replay_store = None
                self._full, self._out = None, {}


def _is(t, torch, dtype, shape, device):
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == device and t.dtype == dtype and t.is_contiguous()
            and tuple(t.shape) == tuple(shape))
