"""Sparse origin demand for the node kernels' quiet paths.  node_kernel<LU> decides per wave -- by a vote over the 64 replica lanes of a
group -- to skip loads (quiet corridors), stores (zero elision) and node arithmetic (lean quiet step); these patterns make the lanes of a
group disagree, one lane at a time, at the group's edges, at different steps, and leave whole groups empty.

Every generator is a function (T, R) -> [R, T] float64 matrix of one origin's demand: deterministic, non-negative integers (and, in
minus_zero alone, zeros with a sign).  `key`
varies the drawn values from origin to origin (never which lanes or steps are busy), `W` is the model's travel-time window."""
import numpy as np

GROUP = 64                                    # replica lanes of one wave
LONE_LANES = ((0, 0), (1, 63), (2, 31))       # lone_lane: (group, busy lane); every further group stays empty


def _rng(tag, key, r=0):
    return np.random.default_rng([tag, int(key), int(r)])


def lone_busy_replicas(R):
    """Busy replica of each group of lone_lane.  In a partly padded last group the lane is the group's last real replica: the vote
    then runs over one busy lane, quiet lanes in front of it and padding lanes behind it."""
    out = []
    for g, lane in LONE_LANES:
        if g * GROUP < R:
            out.append(min(g * GROUP + lane, R - 1))
    return out


def lone_lane(T, R, key=0, W=10):
    """One busy lane per 64-replica group (lane 0 of group 0, lane 63 of group 1, lane 31 of group 2), every other replica and every
    further group zero over the whole horizon.  The busy lanes get a short Poisson pulse."""
    d = np.zeros((R, T))
    for r in lone_busy_replicas(R):
        d[r, 1:9] = 1 + _rng(1, key, r).poisson(7.0, 8)
    return d


def staggered_start(r):
    return 1 + (7 * r) % 60


def staggered(T, R, key=0, W=10):
    """Replica r gets a 6-step pulse from step 1 + (7 r) % 60: the lanes of a group turn busy, and quiet again, at different steps."""
    d = np.zeros((R, T))
    for r in range(R):
        s = staggered_start(r)
        n = max(0, min(6, T - s))
        d[r, s:s + n] = 1 + _rng(2, key, r).poisson(8.0, 6)[:n]
    return d


DRAIN_PULSE = 3      # steps of each of drain_refill's two pulses


def drain_silences(W):
    return (W - 1, W, W + 1, 2 * W)


def drain_second_pulse(r, W):
    """first step of replica r's second pulse"""
    return 1 + DRAIN_PULSE + drain_silences(W)[r % 4]


def drain_refill(T, R, key=0, W=10):
    """A pulse, a silence, a second pulse.  During the silence the corridors next to the origin empty while their cumulative counts stay
    non-zero and level -- such a corridor is not quiet -- and the moving travel-time window, whose oldest entry the link update of step
    t - 1 reads at row t - 1 - W, runs out of the first pulse: the silences last W - 1, W, W + 1 and 2 W steps (replica r: entry r % 4)."""
    d = np.zeros((R, T))
    for r in range(R):
        g = _rng(3, key, r)
        d[r, 1:1 + DRAIN_PULSE] = 6 + g.poisson(10.0, DRAIN_PULSE)
        s = drain_second_pulse(r, W)
        d[r, s:s + DRAIN_PULSE] = 6 + g.poisson(10.0, DRAIN_PULSE)
    return d


def single_ped_step(r):
    return 1 + (5 * r) % 23


def single_ped(T, R, key=0, W=10, peds=1.0):
    """A demand of exactly 1.0 at one step per replica, step 1 + (5 r) % 23, and nothing else: the smallest non-zero state there is.
    (`peds`: the amount, for an origin that splits 1.0 into fractions whose floor is nobody.)"""
    d = np.zeros((R, T))
    for r in range(R):
        d[r, single_ped_step(r)] = peds
    return d


def alternating(T, R, key=0, W=10):
    """Even replicas have demand at odd steps only, odd replicas at even steps only: at every step half of the lanes, interleaved."""
    d = np.zeros((R, T))
    t = np.arange(T)
    for r in range(R):
        on = (t % 2 == 1) if r % 2 == 0 else ((t % 2 == 0) & (t > 0))
        d[r, on] = 1 + _rng(5, key, r).poisson(3.0, int(on.sum()))
    return d


def all_zero(T, R, key=0, W=10):
    """No demand anywhere: every vote of every step comes out quiet."""
    return np.zeros((R, T))


def minus_zero(T, R, key=0, W=10):
    """all_zero to every comparison of numbers, but lone_lane's busy lanes carry -0.0 at steps 1..5.  A one-to-one origin passes
    min(-0.0, r) = -0.0 on as the inflow of its corridor, so rows that are zero in all 64 lanes still differ from +0.0 by a sign bit:
    zero elision, which is defined on bits, has to store them."""
    d = np.zeros((R, T))
    for r in lone_busy_replicas(R):
        d[r, 1:6] = -0.0
    return d


PATTERNS = {"lone_lane": lone_lane, "staggered": staggered, "drain_refill": drain_refill, "single_ped": single_ped,
            "alternating": alternating, "all_zero": all_zero}
EXTRA = {"minus_zero": minus_zero}      # a case of its own (long_corridor), not part of the pattern x network matrix
