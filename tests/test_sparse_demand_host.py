"""The sparse-demand patterns through the CPU oracle alone: the preconditions that make test_gpu_sparse_activity.py mean something.  Every
case of that file runs here first -- same network, pattern, replica count and steps -- and must raise no error flag in any replica (so
the GPU side has nothing to skip), take the sending-flow paths, and show the state its pattern is there for."""
import numpy as np
import pytest

import sparse_demand as sd
import sparse_oracle as so
from fuzz_cases import random_case
from pednstream_amd.flatten import flatten_network

ZERO_FIELDS = ("inflow", "outflow", "cumulative_inflow", "cumulative_outflow", "num_pedestrians", "density", "link_flow")   # +0.0 while empty


def run(pattern, name, R, steps=None):
    net = so.build(name, R)
    demand = so.demand_for(net, pattern, R, name)
    steps = so.steps_for(pattern, so.window(net)) if steps is None else steps
    o = so.Oracles(net, demand, R)
    o.run(1, steps)
    return net, demand, o, steps


def plus_zero(a):
    return not so.bits(a).any()


@pytest.mark.parametrize("name,seed,short", [("fuzz_separators", so.FUZZ_SEPARATORS, False), (so.SHORT_LINKS, so.FUZZ_SHORT_LINKS, True)])
def test_fuzz_seeds_have_separators_and_static_fractions(name, seed, short):
    adj, params, origins, dests = random_case(seed, short_links=short)
    assert so.fuzz_case(name) == (seed, short)
    assert dests == [] and sum(v.get("controller_type") == "separator" for v in params["links"].values()) >= 1
    m = flatten_network(so.build(name, 1))
    assert int(m["n_od"]) == 0 and not np.asarray(m["node_dyn"]).any()          # no device-computed turning fractions
    assert np.asarray(m["link_sep"]).any()
    assert (np.asarray(m["node_kind"]) == 1).any()                               # junctions: the column pass and row sums exist
    assert ((np.asarray(m["link_tau_sw"]) == 0).any()) == short


def test_steps_stay_short_of_the_horizon():
    for pattern, name, R in so.cases():
        net = so.build(name, 1)
        W = so.window(net)
        assert W + 40 <= so.steps_for(pattern, W) < net.simulation_steps
    assert {R for _, _, R in so.cases()} == set(so.REPLICAS)
    assert max(R for _, n, R in so.cases() if n == "melbourne") <= 192


@pytest.mark.parametrize("pattern,name,R", so.cases())
def test_oracle_meets_the_preconditions(pattern, name, R):
    net, demand, o, steps = run(pattern, name, R)
    W = so.window(net)
    for rows in demand.values():
        assert rows.shape == (R, net.simulation_steps) and (rows >= 0).all() and not np.signbit(rows).any() and np.array_equal(rows, np.floor(rows))
    assert not o.flags().any(), o.flags()
    calls, past_gate, positive, _, _ = o.tally()
    assert calls > 0 and past_gate > 0
    assert (positive > 0) == (pattern != "all_zero")
    q, ci = o.field("inflow", steps), o.field("cumulative_inflow", steps)
    if pattern == "all_zero":
        for f in ZERO_FIELDS:
            assert plus_zero(o.field(f, steps)), f
    if pattern == "lone_lane":
        busy = sd.lone_busy_replicas(R)
        assert busy == {64: [0], 70: [0, 69], 192: [0, 127, 159]}[R]
        idle = np.setdiff1d(np.arange(R), busy)
        for f in ZERO_FIELDS:
            assert plus_zero(o.field(f, steps)[:, :, idle]), f
        assert (ci[-1][:, busy].sum(axis=0) > 0).all()
    if pattern == "staggered":
        started = [r for r in range(R) if sd.staggered_start(r) + 1 < steps]
        assert len(started) == R and (ci[-1].sum(axis=0) > 0).all()       # every lane turns busy inside the run, at its own step
        first = np.array([np.flatnonzero(q[:, :, r].sum(axis=1))[0] for r in range(R)])
        assert np.array_equal(first, [sd.staggered_start(r) + 1 for r in range(R)])
    if pattern == "drain_refill":
        assert sorted(set(sd.drain_silences(W))) == sorted({W - 1, W, W + 1, 2 * W})
        for r in range(R):
            s = sd.drain_second_pulse(r, W)        # its demand enters at step s + 1
            level = (ci[s, :, r] > 0) & (q[s, :, r] == 0)
            again = q[s + 1:s + 1 + sd.DRAIN_PULSE, :, r].sum(axis=0) > 0
            assert (level & again).any(), r
    if pattern == "single_ped":
        assert (q == 1.0).any()
        for rows in demand.values():
            assert ((rows > 0).sum(axis=1) == 1).all() and rows.max() == so.SINGLE_PED.get(name, 1.0)
        assert len({sd.single_ped_step(r) for r in range(R)}) == 23
    if pattern == "alternating":
        t = np.arange(net.simulation_steps)
        for rows in demand.values():
            assert not rows[0::2][:, t % 2 == 0].any() and not rows[1::2][:, t % 2 == 1].any()
    o.close()


def test_lone_lane_leaves_a_whole_group_at_plus_zero():
    """256 replicas (the two-chain case): the fourth group has no busy lane and every field that is zero while a corridor is empty
    holds +0.0 by bits in it, every row"""
    net, demand, o, steps = run("lone_lane", "fuzz_separators", 256)
    assert sd.lone_busy_replicas(256) == [0, 127, 159] and not o.flags().any()
    for f in ZERO_FIELDS:
        assert plus_zero(o.field(f, steps)[:, :, 192:]), f
    assert o.field("cumulative_inflow", steps)[-1][:, [0, 127, 159]].sum() > 0
    o.close()


@pytest.mark.parametrize("R", [70, 192])
def test_minus_zero_reaches_the_histories(R):
    """long_corridor's origins are one-to-one nodes: a demand of -0.0 arrives as an inflow of -0.0, everything else stays +0.0"""
    net, demand, o, steps = run("minus_zero", "long_corridor", R)
    assert not o.flags().any()
    q = o.field("inflow", steps)
    minus = np.signbit(q) & (q == 0)
    assert minus.any() and sorted(np.unique(np.argwhere(minus)[:, 2])) == sd.lone_busy_replicas(R)
    for f in ZERO_FIELDS:
        assert not o.field(f, steps).any(), f                       # zero as numbers ...
        assert plus_zero(o.field(f, steps)) == (f != "inflow"), f     # ... and by bits all but the inflow
    o.close()


@pytest.mark.parametrize("pattern", ["all_zero", "lone_lane"])
def test_short_links_raise_the_same_step_flag_in_every_replica(pattern):
    """why the network with short links is compared by this flag alone (sparse_oracle.SHORT_LINKS)"""
    net, demand, o, steps = run(pattern, so.SHORT_LINKS, 70)
    assert (o.flags() & so.F_SAME_STEP).all()
    o.close()
