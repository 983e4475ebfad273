"""The replay contract without a GPU: the ring of tests/replay_model.py (what pednstream_amd/csrc/pedn_replay.hpp must hold) hands out
exactly what the reference's deques hold (rl/agents/SAC.py:148-198 over rl/rl_utils.py:37-50), and its draws are the Philox words of
oracle/rng_contract.py."""
import os
import sys

import numpy as np
import pytest

import replay_model as rp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rng_contract as rc  # noqa: E402

E = 30                      # policy steps of an episode (the T_SHORT of the GPU tests' env)
N, O, A, NA = 3, 5, 2, 3    # envs, observation / action columns, agents


def feed(models, capacity, episodes, early_reset_after=None, seed=0):
    """The same synthetic episodes into every model; ``early_reset_after``: the second episode is cut after that many steps."""
    rng = np.random.default_rng(seed)
    for ep in range(episodes):
        steps = early_reset_after if (early_reset_after is not None and ep == 1) else E
        obs = rng.standard_normal((N, O)).astype(np.float32)
        for m in models:
            m.begin(obs)
        for t in range(steps):
            obs, act = rng.standard_normal((N, O)).astype(np.float32), rng.standard_normal((N, A))
            rew = rng.standard_normal((N, NA)).astype(np.float32)
            for m in models:
                m.push(obs, act, rew, t == E - 1)
            yield


def ring_transitions(ring, e):
    return [ring.transition(s, e) for s in ring.sampleable()]


def same_transitions(a, b):
    return len(a) == len(b) and all(all(np.array_equal(x, y) for x, y in zip(ta, tb)) for ta, tb in zip(a, b))


@pytest.mark.parametrize("stack", [1, 2, 4])
@pytest.mark.parametrize("capacity", [1, 5, 2 * E + 1])
def test_ring_holds_what_the_deques_hold(capacity, stack):
    ring, ref = rp.RingModel(capacity, stack, E, N), rp.DequeModel(capacity, stack, N)
    assert ring.R == capacity + stack + -(-capacity // E) + 1
    pushed = 0
    for _ in feed((ring, ref), capacity, episodes=6):
        pushed += 1
        assert ring.size_rows == min(pushed, capacity)          # full-length episodes: deque(maxlen) exactly
        assert np.array_equal(ring.stacked_obs(), np.stack([ref.state_stack[e] for e in range(N)]))
        if pushed % 7 == 0 or pushed > 6 * E - 3:
            for e in range(N):
                assert same_transitions(ring_transitions(ring, e), list(ref.buffer[e]))
    assert pushed == 6 * E and ring.head == pushed + 6 > 2 * ring.R          # (the ring has wrapped more than twice)


@pytest.mark.parametrize("stack", [1, 2, 4])
@pytest.mark.parametrize("capacity", [1, 5, 2 * E + 1])
def test_an_early_reset_leaves_a_suffix_of_the_deque(capacity, stack):
    ring, ref = rp.RingModel(capacity, stack, E, N), rp.DequeModel(capacity, stack, N)
    for _ in feed((ring, ref), capacity, episodes=4, early_reset_after=2):
        assert np.array_equal(ring.stacked_obs(), np.stack([ref.state_stack[e] for e in range(N)]))
        for e in range(N):
            mine, theirs = ring_transitions(ring, e), list(ref.buffer[e])
            assert len(mine) <= len(theirs) and same_transitions(mine, theirs[len(theirs) - len(mine):])
    assert ring.size_rows == len(ring.sampleable()) >= 1


def test_indices_are_the_philox_words():
    seed, n_envs, jhead, size = 0x1234_5678_9ABC_DEF0, 65, 41, 17
    for d in (0, 1, (1 << 32) + 5):
        got = rp.draw_indices(seed, d, 9, jhead, size, n_envs)
        for k in range(9):
            w = rc.philox4x32_10((k, d % 2 ** 32, 0x71, d // 2 ** 32), (seed % 2 ** 32, seed // 2 ** 32))
            assert got[k, 0] == jhead - 1 - (w[0] * size) // 2 ** 32 and got[k, 1] == (w[1] * n_envs) // 2 ** 32
            assert jhead - size <= got[k, 0] < jhead and 0 <= got[k, 1] < n_envs
    ring = rp.RingModel(5, 2, E, N, seed=seed)
    for _ in feed((ring,), 5, episodes=1):
        pass
    first, second = ring.draw(8), ring.draw(8)
    assert ring.draws == 2 and not np.array_equal(first, second)
    je = rp.draw_indices(seed, 1, 8, ring.jhead, ring.size_rows, N)
    assert np.array_equal(second[:, 0], ring.step_serial[je[:, 0] % 5]) and np.array_equal(second[:, 1], je[:, 1])
    assert all(ring.is_sampleable(int(s)) for s in second[:, 0])


def test_draws_are_uniform_over_rows_and_envs():
    size, n_envs, draws = 7, 3, 21000
    je = rp.draw_indices(7, 0, draws, 100, size, n_envs)
    counts = np.zeros((size, n_envs), dtype=np.int64)
    np.add.at(counts, (99 - je[:, 0], je[:, 1]), 1)
    # five standard deviations of a binomial with p = 1 / 21: sqrt(21000 * (1 / 21) * (20 / 21)) = 30.9
    assert counts.sum() == draws and np.abs(counts - 1000).max() <= 155, counts
