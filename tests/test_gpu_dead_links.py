"""Dead-link plan of pedn_run (PEDN_DEAD_LINKS; pedn_partition.hpp, dead_link_kernel, launch_split_step): in a two-chain range the nodes
that provably never see a pedestrian are stepped by the lean kernel, node_kernel<LU> runs over the other nodes only on a third stream.

The network is small on purpose: 12 nodes, one origin, and one turning fraction of exactly 0.0 at junction 2 that closes the branch
behind it -- 13 dead links and 4 dead virtual pairs, 17 slot waves per replica group (not a multiple of the 4 waves of a workgroup, nor
of the 8 of a bin).

    0 - 1 - 2 - 3 - 4          the live path (origin 0)
            |
            5 - 10             5, 6, 8: junctions; 7, 9, 10, 11: dead ends (a virtual pair each, demand row zero)
            |
            6 - 7
            |
            8 - 9
            |
            11

Yardsticks: the same engine with PEDN_DEAD_LINKS=0 driven through the same calls -- every history field, every row, column and replica
by bits, and the error flags (the running sum has no reader of its own: every avg_travel_time row from step W on is a function of it,
and the steps that follow a change of plan continue from it; the issue asks for the running sum itself, which the C-ABI does not
hand out) -- and the CPU oracle on a sample of replicas."""
import os

import numpy as np
import pytest

import dead_link_cases as dl
import sparse_demand as sd
from dead_link_cases import KEYS
from golden_util import ALL_FIELDS
from sparse_oracle import assert_same_bits

pytestmark = pytest.mark.gpu

EDGES = [(0, 1), (1, 2), (2, 3), (3, 4), (2, 5), (5, 6), (6, 7), (6, 8), (8, 9), (5, 10), (8, 11)]
N_NODES, STEPS, SEED = 12, 41, 9
DEAD_LINKS = 13          # head node in {5 .. 11}


def tree(origins=(0,)):
    """(adj, params, origins, dests) of the 12-node tree"""
    adj = np.zeros((N_NODES, N_NODES), dtype=int)
    for a, b in EDGES:
        adj[a, b] = adj[b, a] = 1
    params = {"unit_time": 10.0, "simulation_steps": 60, "assign_flows_type": "classic", "seed": SEED,
              "default_link": {"length": 60.0, "width": 3.0, "free_flow_speed": 1.3, "k_critical": 2.0, "k_jam": 6.0, "gamma": 0.01,
                               "speed_noise_std": 0.03, "fd_type": "yperman", "bi_factor": 1.0, "activity_probability": 0.1},
              "links": {}, "demand": {f"origin_{o}": {"pattern": "constant", "peak_lambda": 10.0, "base_lambda": 5.0} for o in origins}}
    return adj, params, list(origins), []


def Pair(R, history="full", oracle=True, knobs=None):
    """dead_link_cases.Pair on the tree: the same network with the plan on and off, and one CPU oracle per sampled replica"""
    return dl.Pair(tree(), R, SEED, history=history, oracle=oracle, knobs=knobs)


def start(R, **kw):
    p = Pair(R, **kw)
    p.tf(2, 1, 5)                  # nobody turns from 1 -> 2 into 2 -> 5: the branch behind junction 2 is dead
    p.demand(0, sd.staggered(p.T, R, key=3))
    return p


@pytest.mark.parametrize("R,streams,waves", [(320, 1, 5), (330, 2, 5), (384, 2, 8), (320, 1, 3)])
def test_ranges_that_switch_plans(R, streams, waves):
    """3 steps on one chain, 20 split, single steps, 20 split again: 320 / 384 replicas are halves of 256 + 128, 330 leaves a group
    with padding lanes.  The lean kernel as one launch per step for the whole batch (the default) and as one per half on the two chain
    streams, at the default share of the wave places, without a limit (8) and at the smallest one (3)."""
    p = start(R, knobs={"PEDN_DEAD_STREAMS": str(streams), "PEDN_DEAD_WAVES": str(waves)})
    assert p.dead() == DEAD_LINKS
    p.run(1, 4)
    assert p.split_steps() == 0              # a range of one chain
    p.run(4, 24)
    assert p.split_steps() == 19             # the first node launch of the range stays on the full bin set
    p.check(24, f"x {R}: after the first split range")
    for t in range(24, 27):
        p.step(t)
    assert p.split_steps() == 19
    p.run(27, 47)
    assert p.split_steps() == 38
    p.check(47, f"x {R}: at the end")
    assert p.dead() == DEAD_LINKS
    p.close()


def test_melbourne_as_the_benchmark_builds_it():
    """The engine's own derivation of the proof's inputs (demand rows scanned at upload, host-tabulated rows of the four dynamic nodes)
    on the headline model: 916 links with their head node among the 333 that nobody reaches -- the figure tests/test_partition_host.py
    gets from the Python restatement -- and a split range equal to the unsplit one by bits."""
    from golden_util import DATA
    from pednstream_amd import NetworkEnvGenerator
    from test_gpu_quiet_corridors import poisson_demand

    R, steps = 256, 14
    engines = []
    keep = {k: os.environ.get(k) for k in KEYS}
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


def test_upload_into_a_zero_row_shrinks_the_set_mid_episode():
    p = start(320)
    p.tf(6, 7, 8)                  # ... and from 7 -> 6 nobody turns into 6 -> 8: 8, 9, 11 stay dead when 7 becomes an origin
    p.run(1, 21)
    assert p.dead() == DEAD_LINKS
    rows = sd.lone_lane(p.T, 320, key=5)
    rows[:, :25] = 0.0
    rows[::7, 25:31] = 3.0
    p.demand(7, rows)
    left = p.dead()
    assert left == 5, left         # 6 -> 8, 9 -> 8, 11 -> 8, 8 -> 9, 8 -> 11
    p.run(21, STEPS)
    p.check(STEPS, "demand into node 7 at step 21")
    p.close()


def test_pedestrians_on_their_way_stay_a_source_when_their_origin_is_zeroed():
    """Found by tests/test_gpu_dead_links_random.py (seed 4481): the origin's row is zeroed in every replica while its pedestrians are
    between nodes 0 and 2, then the turn 1 -> 2 -> 5 opens in front of them.  A proof that starts from the demand rows alone has no source
    left and keeps the branch dead; the links reached so far are sources too, and the whole branch goes back to the node kernel."""
    p = start(320)
    p.run(1, 21)
    assert p.dead() == DEAD_LINKS
    p.set_demand(p.index[0], np.zeros(p.T + 1))
    assert p.dead() == DEAD_LINKS
    n = p.index[2]
    d = int(p.model["node_slot_ptr"][n + 1] - p.model["node_slot_ptr"][n])
    p.set_tf(n, np.full(d * (d - 1), 1.0 / (d - 1)))
    assert p.dead() == 0
    p.run(21, STEPS)
    p.check(STEPS, "origin zeroed at step 21, then the closed turn opened")
    branch = p.net.links[(2, 5)].index
    assert p.on.read_block(0, 21, STEPS, branch, branch + 1).any()          # somebody did turn into the branch
    p.close()


def test_lazy_reset_never_grows_the_set_a_full_reset_does():
    p = start(320)
    p.run(1, 21)
    for e in (p.on, p.off):
        e.reset(lazy=True)
    for o in p.oracles:
        o.reset()
    p.demand(0, np.zeros((320, p.T)))            # the second episode's origin is node 7
    p.demand(7, sd.staggered(p.T, 320, key=11))
    assert p.dead() == 0                         # what was live in the first episode stays with the node kernel, and now the rest is live too
    p.run(1, STEPS)
    p.check(STEPS, "second episode after a lazy reset")
    for e in (p.on, p.off):
        e.reset()
    for o in p.oracles:
        o.reset()
    p.tf(6, 7, 8)
    assert p.dead() == 5                         # a full reset: proven afresh, for the origin at node 7
    p.run(1, STEPS)
    p.check(STEPS, "third episode after a full reset")
    p.close()


@pytest.mark.parametrize("value", [-1.0, float("nan")])
def test_gate_setter_on_a_dead_link(value):
    p = start(320, oracle=value == value)
    link = p.net.links[(6, 8)].index
    p.run(1, 15)
    before = p.dead()
    p.width(1, link, value)                      # back gate of 6 -> 8: the corridor 6 - 8 goes back to the node kernel, and nodes 6 and 8 with it
    assert 0 < p.dead() < before
    p.run(15, STEPS)
    p.check(STEPS, f"back gate {value} on a dead link")
    p.close()


def test_a_device_pointer_turns_the_plan_off_until_a_full_reset():
    p = start(320, oracle=False)
    p.run(1, 15)
    assert p.dead() == DEAD_LINKS
    for e in (p.on, p.off):
        assert e.device_ptr(0)[0]
    assert p.dead() == 0
    p.run(15, STEPS)
    p.check(STEPS, "after a zero-copy pointer")
    for e in (p.on, p.off):
        e.reset(lazy=True)
    assert p.dead() == 0
    for e in (p.on, p.off):
        e.reset()
    assert p.dead() == DEAD_LINKS
    p.close()


def test_no_dead_link_no_split():
    p = Pair(320, oracle=False)                  # uniform fractions: every node is reached
    p.demand(0, sd.staggered(p.T, 320, key=3))
    assert p.dead() == 0
    p.run(1, STEPS)
    p.check(STEPS, "no dead link")
    p.close()


def test_recent_history_keeps_the_plan_off():
    p = start(320, history="recent", oracle=False)
    assert p.dead() == 0
    p.close()


def test_live_slot_next_to_a_dead_corridor_goes_quiet_and_busy_again():
    """Junction 2's slot of the corridor 2 - 5 mirrors itself in the live packing.  Demand in two pulses with a silence longer than the
    network takes to drain: its quiet words switch on, off and on again while the dead end of the corridor never writes one."""
    p = start(384)
    rows = np.zeros((384, p.T))
    rows[:, 1:4] = 4.0
    rows[5::64, 26:29] = 6.0
    p.demand(0, rows)
    p.run(1, STEPS)
    p.check(STEPS, "two pulses")
    live = p.net.links[(5, 2)].index             # stepped by node 2's slot wave; its reverse 2 -> 5 by the lean kernel
    assert not p.on.read_block(0, 0, STEPS, live, live + 1).any() and p.on.read_block(2, 0, STEPS)[:, :p.on.n_links].any()
    p.close()
