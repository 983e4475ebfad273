"""The replay contract restated in numpy -- what pednstream_amd/csrc/pedn_replay.hpp must hold and hand out bit for
bit -- and, independently of it, the reference's own bookkeeping: a ``collections.deque(maxlen=stack_size)`` of observations and a
``collections.deque(maxlen=capacity)`` of (state_stack, action, reward, next_state_stack, done) per env, fed the way
train_off_policy_multi_agent feeds them (rl/agents/SAC.py:148-198, rl/rl_utils.py:37-50).

    m = RingModel(capacity, stack_size, episode_steps, n_envs, seed)
    m.begin(obs); m.push(obs, actions, rewards, done); m.stacked_obs(); m.size_rows
    m.sampleable()                     # serials, oldest first
    m.gather(idx)                      # (states, actions, rewards, next_states, dones) of [B, 2] (serial, env) pairs
    m.draw(B)                          # the indices of the next sample(B) call; advances the draw counter
"""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
from rng_contract import philox4x32_10  # noqa: E402

DRAW_SITE = 0x71


def ring_slots(capacity, stack_size, episode_steps):
    return capacity + stack_size + -(-capacity // episode_steps) + 1


def draw_indices(seed, d, batch, jhead, size_rows, n_envs):
    """[batch, 2] (STEP count j, env) of draw d."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty((batch, 2), dtype=np.int64)
    for k in range(batch):
        w = philox4x32_10((k, d & 0xFFFFFFFF, DRAW_SITE, (d >> 32) & 0xFFFFFFFF), key)
        out[k] = jhead - 1 - ((w[0] * size_rows) >> 32), (w[1] * n_envs) >> 32
    return out


class RingModel:
    def __init__(self, capacity, stack_size, episode_steps, n_envs, seed=0):
        self.cap, self.S, self.N, self.seed = int(capacity), int(stack_size), int(n_envs), int(seed)
        self.R = ring_slots(self.cap, self.S, int(episode_steps))
        self.frames = [None] * self.R          # per slot: [n_envs, n_obs] float32
        self.actions = [None] * self.R
        self.rewards = [None] * self.R
        self.done = np.zeros(self.R, dtype=np.float32)
        self.first = np.zeros(self.R, dtype=np.int64)
        self.serial_of = np.zeros(self.R, dtype=np.int64)          # (the model's own check that a slot still holds what is asked for)
        self.step_serial = np.zeros(self.cap, dtype=np.int64)
        self.head = self.jhead = self.size_rows = self.draws = 0
        self.cur_first = -1

    # ------------------------------------------------------------------------------------------------ rows
    def _row(self, obs):
        s = self.head
        slot = s % self.R
        self.frames[slot] = np.array(obs, dtype=np.float32, copy=True)
        self.serial_of[slot] = s
        return s, slot

    def _oldest_frame(self, s):
        return max(s - self.S, int(self.first[s % self.R]))

    def _advance(self):
        self.head += 1
        dropped = 0
        while self.size_rows > 0 and self._oldest_frame(int(self.step_serial[(self.jhead - self.size_rows) % self.cap])) < self.head - self.R:
            self.size_rows -= 1
            dropped += 1
        assert dropped <= self.S + 1          # the bound of the kernel's loop

    def begin(self, obs):
        s, slot = self._row(obs)
        self.first[slot] = -1
        self.cur_first = s
        self._advance()

    def push(self, obs, actions, rewards, done):
        assert self.cur_first >= 0
        s, slot = self._row(obs)
        self.actions[slot] = np.array(actions, dtype=np.float64, copy=True)
        self.rewards[slot] = np.array(rewards, dtype=np.float32, copy=True)
        self.done[slot] = 1.0 if done else 0.0
        self.first[slot] = self.cur_first
        self.step_serial[self.jhead % self.cap] = s
        self.jhead += 1
        self.size_rows = min(self.size_rows + 1, self.cap)
        self._advance()

    # ------------------------------------------------------------------------------------------------ stacks
    def frame(self, x):
        assert self.head - self.R <= x < self.head and self.serial_of[x % self.R] == x, "a frame outside the ring"
        return self.frames[x % self.R]

    def stack(self, s, q, shift):
        """[n_envs, stack, n_obs]: the frames max(s - stack + shift + i, q)."""
        return np.stack([self.frame(max(s - self.S + shift + i, q)) for i in range(self.S)], axis=1)

    def stacked_obs(self):
        s = self.head - 1
        q = int(self.first[s % self.R])
        return self.stack(s, s if q < 0 else q, 1)

    def sampleable(self):
        return [int(self.step_serial[j % self.cap]) for j in range(self.jhead - self.size_rows, self.jhead)]

    def is_sampleable(self, s):
        return s in self.sampleable()

    def transition(self, s, e):
        slot = s % self.R
        q = int(self.first[slot])
        assert q >= 0 and self.serial_of[slot] == s
        return (self.stack(s, q, 0)[e], self.actions[slot][e], self.rewards[slot][e], self.stack(s, q, 1)[e], self.done[slot])

    def gather(self, idx, obs=slice(None), act=slice(None), rew=slice(None)):
        rows = [self.transition(int(s), int(e)) for s, e in np.asarray(idx)]
        st, a, r, ns, d = zip(*rows)
        return (np.stack(st)[..., obs], np.stack(a)[..., act], np.stack(r)[..., rew], np.stack(ns)[..., obs], np.array(d, dtype=np.float32))

    # ------------------------------------------------------------------------------------------------ drawing
    def draw(self, batch):
        assert self.size_rows > 0
        je = draw_indices(self.seed, self.draws, batch, self.jhead, self.size_rows, self.N)
        self.draws += 1
        return np.stack([self.step_serial[je[:, 0] % self.cap], je[:, 1]], axis=1)


class DequeModel:
    """The reference's loop for a batch of envs: per env a deque of the last ``stack_size`` observations and a replay deque."""

    def __init__(self, capacity, stack_size, n_envs):
        self.S, self.N = stack_size, n_envs
        self.history = [collections.deque(maxlen=stack_size) for _ in range(n_envs)]
        self.buffer = [collections.deque(maxlen=capacity) for _ in range(n_envs)]
        self.state_stack = [None] * n_envs

    def begin(self, obs):
        for e in range(self.N):
            self.history[e].clear()
            for _ in range(self.S):
                self.history[e].append(np.array(obs[e], copy=True))
            self.state_stack[e] = np.array(self.history[e])

    def push(self, obs, actions, rewards, done):
        for e in range(self.N):
            self.history[e].append(np.array(obs[e], copy=True))
            nxt = np.array(self.history[e])
            self.buffer[e].append((self.state_stack[e], np.array(actions[e], copy=True), np.array(rewards[e], copy=True), nxt, np.float32(1.0 if done else 0.0)))
            self.state_stack[e] = nxt
