"""The dead links of a split range in blocks of steps per launch (PEDN_DEAD_BLOCK; lean_block_kernel, launch_split_block,
pedn_plan::dead_block_len): one lean launch performs up to min(K, W) steps with a lane's running sum and previous receiving flow in
registers, the live launches beside it go out step by step as before.

The network, the calls and the yardsticks are those of tests/test_gpu_dead_links.py: the 12-node tree (W = 10, 17 dead slot waves per
replica group), the same engine with PEDN_DEAD_LINKS=0 driven through the same calls -- every field, row, column and replica by bits, and
the error flags -- and the CPU oracle on a sample of replicas; 320 replicas, and 330 with padding lanes.  The steps launched under the plan
must be those of an engine with PEDN_DEAD_BLOCK=1 (one launch per step): the planner still plans and commits every step.

pedn_run gives a range of fewer than 8 steps one chain (dead_link_cases.MIN_CHAIN_RANGE), so no range of two steps is ever split: the
two-step range below checks exactly that, and the block of ONE step behind a full block -- which dead_link_kernel performs -- comes from a
block length of 6 on the shortest split range there is, 1 full step + 7 split ones."""
import os

import numpy as np
import pytest

import dead_link_cases as dl
import sparse_demand as sd
from golden_util import ALL_FIELDS
from sparse_oracle import assert_same_bits
from test_gpu_dead_links import DEAD_LINKS, SEED, STEPS, tree

pytestmark = pytest.mark.gpu

BLOCK_KEYS = ("PEDN_DEAD_BLOCK", "PEDN_DEAD_BLOCK_WAVES")


def start(R, block, streams=1, waves=None, oracle=True, case=None):
    """test_gpu_dead_links.start with the block knobs, which leave the environment as they found it"""
    keep = {k: os.environ.get(k) for k in BLOCK_KEYS}
    knobs = {"PEDN_DEAD_STREAMS": str(streams)}
    if block is not None:
        knobs["PEDN_DEAD_BLOCK"] = str(block)
    if waves is not None:
        knobs["PEDN_DEAD_BLOCK_WAVES"] = str(waves)
    try:
        p = dl.Pair(case or tree(), R, SEED, oracle=oracle, knobs=knobs)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    p.tf(2, 1, 5)                  # nobody turns from 1 -> 2 into 2 -> 5: the branch behind junction 2 is dead
    p.demand(0, sd.staggered(p.T, R, key=3))
    return p


def switching_calls(p, counts=None):
    """the calls of test_ranges_that_switch_plans; the steps launched under the plan after each"""
    out = []
    p.run(1, 4)
    out.append(p.split_steps())
    p.run(4, 24)
    out.append(p.split_steps())
    if counts is not None:
        p.check(24, "after the first split range")
    for t in range(24, 27):
        p.step(t)
    out.append(p.split_steps())
    p.run(27, 47)
    out.append(p.split_steps())
    if counts is not None:
        p.check(47, "at the end")
        assert out == counts, (out, counts)
    return out


@pytest.fixture(scope="module")
def per_step_counts():
    """split_steps() of an engine with one lean launch per step, after each of the calls"""
    p = start(320, 1, oracle=False)
    counts = switching_calls(p)
    p.close()
    assert counts == [0, 19, 19, 38]
    return counts


@pytest.mark.parametrize("block", [2, 7, 10])
@pytest.mark.parametrize("R,streams", [(320, 1), (330, 2)])
def test_ranges_that_switch_plans_in_blocks(R, streams, block, per_step_counts):
    """3 steps on one chain, 20 split, single steps, 20 split again.  The 19 split steps of a range are no multiple of 7 (7 + 7 + 5), and
    the switches t' >= fft (5) and t' >= W (10) fall inside the first block of 7 and of 10 (t' = 4 .. 10 / 4 .. 13)."""
    p = start(R, block, streams)
    assert p.dead() == DEAD_LINKS
    switching_calls(p, per_step_counts)
    assert p.dead() == DEAD_LINKS
    p.close()


def test_a_range_of_two_steps_and_the_shortest_split_range():
    """blocks of 6 on 7 split steps: one block kernel launch and one block of a single step; blocks of 10: a range shorter than K"""
    for block in (6, 10):
        p = start(320, block)
        p.run(1, 3)
        assert p.split_steps() == 0              # two steps: one chain, as without blocks
        p.run(3, 3 + dl.MIN_CHAIN_RANGE)
        assert p.split_steps() == dl.MIN_CHAIN_RANGE - 1
        p.run(11, 13)
        assert p.split_steps() == dl.MIN_CHAIN_RANGE - 1
        p.run(13, 24)                            # t' >= W inside the single block of 10
        assert p.split_steps() == dl.MIN_CHAIN_RANGE - 1 + 10
        p.check(24, f"blocks of {block}")
        p.close()


def test_a_block_longer_than_the_window_is_cut_to_the_window():
    """PEDN_DEAD_BLOCK=16 on W = 10: a block of 16 steps would read travel_time rows that it writes itself (avg_travel_time from t' = 10 on)"""
    p = start(330, 16, streams=2)
    p.run(1, STEPS)
    assert p.split_steps() == STEPS - 2
    p.check(STEPS, "PEDN_DEAD_BLOCK=16, W = 10")
    p.close()


def test_a_window_of_two_steps():
    adj, params, origins, dests = tree()
    params["unit_time"] = 50.0
    p = start(320, 10, case=(adj, params, origins, dests))
    assert int(p.model["window"]) == 2 and p.dead() == DEAD_LINKS
    p.run(1, STEPS)
    assert p.split_steps() == STEPS - 2
    p.check(STEPS, "unit_time 50: W = 2")
    p.close()


def test_zero_gates_that_change_inside_a_block():
    """an episode to t = 20, a lazy reset, then 39 steps: the rows up to the first episode's last keep their marks, so the gates of the
    block that crosses them are neither all open nor all closed"""
    p = start(320, 10)
    p.run(1, 20)
    p.check(20, "first episode")
    p.reset(lazy=True)
    p.run(1, 40)
    assert p.split_steps() == 38
    gated = p.on.plan_info()["zero_elide_launches"]
    assert 0 < gated < 2 * 38, gated          # (two launches per split step) some steps of the second episode had a gate, some had none
    p.check(40, "second episode after a lazy reset")
    p.close()


def test_a_gate_setter_between_two_ranges_gives_the_blocks_a_new_record():
    p = start(320, 7)
    link = p.net.links[(6, 8)].index
    p.run(1, 15)
    before = p.dead()
    p.width(1, link, 1.5)                        # back gate of the dead link 6 -> 8 at another valid width: the set stays, the record changes
    assert p.dead() == before == DEAD_LINKS
    p.run(15, STEPS)
    assert p.split_steps() == 13 + STEPS - 16
    p.check(STEPS, "back gate 1.5 on a dead link")
    p.close()


def test_melbourne_in_default_blocks():
    """tests/test_gpu_dead_links.py's melbourne x 256 over 24 steps at the default block length, against PEDN_DEAD_LINKS=0"""
    from golden_util import DATA
    from pednstream_amd import NetworkEnvGenerator
    from test_gpu_quiet_corridors import poisson_demand

    R, steps = 256, 24
    engines = []
    keep = {k: os.environ.get(k) for k in dl.KEYS}
    try:
        for dead in ("1", "0"):
            os.environ.update({"PEDN_DEAD_LINKS": dead, "PEDN_STREAMS": "2", "PEDN_STREAM_PROBE": "0"})
            np.random.seed(7)
            net = NetworkEnvGenerator(DATA).create_network("melbourne", verbose=False, n_replicas=R, rng_seed=5)
            e = net.engine()
            for nid in net.origin_nodes:
                net.set_demand_matrix(nid, np.stack([poisson_demand(net.simulation_steps, 31 * r + nid) for r in range(R)]))
            engines.append((net, e))
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    (_, on), (_, off) = engines
    assert on.plan_info()["dead_links"] == 916 and off.plan_info()["dead_links"] == 0
    for e in (on, off):
        e.run(1, steps)
    assert on.plan_info()["dead_link_steps"] == steps - 2 and off.plan_info()["dead_link_steps"] == 0
    assert on.error_flags()[1].tobytes() == off.error_flags()[1].tobytes()
    for fid, name in enumerate(ALL_FIELDS):
        assert_same_bits(on.read_block(fid, 0, steps), off.read_block(fid, 0, steps), f"melbourne x {R}: {name}", "[t, column, replica]")
    assert on.read_block(2, steps - 1, steps).sum() > 0          # somebody walks
    for net, _ in engines:
        net.close()
