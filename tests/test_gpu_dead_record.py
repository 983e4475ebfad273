"""dead_link_kernel on the record of its slot-uniform results (DeadRec, filled on the device by dead_prep_kernel whenever dl_refresh runs;
pednstream_amd/csrc/pedn_kernels.hpp, pedn_hip.hip).

The 12-node tree of test_gpu_dead_links.py, whose branch behind junction 2 is dead (13 links, 4 virtual pairs), with the links of that
branch given parameters of their own, so that no two records are alike:

    0 - 1 - 2 - 3 - 4          live
            |
            5 - 10             5, 6, 8: junctions; 7, 9, 10, 11: dead ends
            |
            6 - 7
            |
            8 - 9
            |
            11

unit_time 10 s: W = 10 steps; the default link (60 m, 1.3 m/s, k_c 2, k_j 6) has free_flow_tau 5 and a shock-wave look-back of 9 steps.
Yardsticks, as in test_gpu_dead_links.py: the same engine with PEDN_DEAD_LINKS=0 through the same calls -- every field, row, column and
replica by bits, and the error flags -- and the CPU oracle on replicas {0, 63, 64, R - 1} (dead_link_cases.Pair.check)."""
import os

import numpy as np
import pytest

import dead_link_cases as dl
import sparse_demand as sd
from dead_link_cases import KEYS
from golden_util import ALL_FIELDS
from sparse_oracle import assert_same_bits
from test_gpu_dead_links import DEAD_LINKS, SEED, tree

pytestmark = pytest.mark.gpu

PEDN_F_SAME_STEP = 16
GATE = ALL_FIELDS.index("back_gate_width_data")


def both(a, b, fwd, rev=None):
    """parameters of the two directions of the corridor a - b (a link looks for its own key first, network.py: _link_params)"""
    return {f"{a}_{b}": dict(fwd), f"{b}_{a}": dict(fwd if rev is None else rev)}


# free_flow_tau / shock-wave look-back: 2 / 3 (20 m), 10 / 20 (130 m: the one at W, the other beyond it), 9 / 21 (90 m at 1.0 m/s, k_c 1.5, k_j 5);
# the rest of the branch keeps 5 / 9.  Steps 2 .. 44 of run(1, 45) are split: t' = 1 lies in front of every switch, t' = 43 behind all.
LENGTHS = {**both(5, 6, {"length": 20.0}), **both(6, 8, {"length": 130.0}),
           **both(8, 9, {"length": 90.0, "free_flow_speed": 1.0, "k_jam": 5.0, "k_critical": 1.5})}
# every fd type of the flattener (network.py: FD_TYPES), each on a corridor with one direction free of noise and one with noise.  At
# density +0.0 smulders leaves a float32 speed, the other two the binary64 free-flow speed (speed_base)
FD_TYPES = {**both(5, 6, {"fd_type": "greenshields", "speed_noise_std": 0.0}, {"fd_type": "greenshields", "speed_noise_std": 0.05}),
            **both(6, 7, {"fd_type": "smulders", "speed_noise_std": 0.0}, {"fd_type": "smulders", "speed_noise_std": 0.04}),
            **both(6, 8, {"fd_type": "yperman", "speed_noise_std": 0.0}, {"fd_type": "yperman", "speed_noise_std": 0.03})}
# 5 m at 1.3 m/s without noise: 3.85 s < unit_time / 2, so avg_travel_time / unit_time rounds to 0 -- the same-step flag of the sending
# flow's look-back, in every replica and at every step; the shock-wave look-back is round(0.77) = 1, still eligible.  But free_flow_tau
# is round(0.385) = 0 then, and such a link is NOT empty in the reference's semantics: its sending flow of step 1 is smoothed against
# entry -1 of the history, the untouched tail's -1.0 (link.py:364), floor(-0.2) = -1; the oracle of replica 63 has sending_flow[0 .. 5] of
# 8 -> 11 at -1, -1, 0, 0, 0, 1 and flags 19 (negative sending flow, negative flow, same step).  A free-flow travel time below half a step
# and a dead link exclude each other: dl_refresh takes such a link for a source (before this test, the plan stepped it as empty: inflow of
# node 11's virtual link +0.0 against -1.0 with the plan off).  What is left of the case: the plan refuses, and on = off = oracle.
SAME_STEP = both(8, 11, {"length": 5.0, "speed_noise_std": 0.0})
# The same-step flag in a link that IS dead needs noise: 6.7 m at 1.3 m/s is 5.15 s, free_flow_tau = shock-wave look-back = 1, and from
# t' = W on the average of ten noisy travel times falls below 5 s -- rint(att / 10) = 0 -- in some replicas at some steps, not in others
SAME_STEP_NOISE = both(8, 11, {"length": 6.7, "speed_noise_std": 0.1})
# the two directions of a corridor with different bi_factor and width: area_in != area_out, kb's divisor is not ka's
ASYMMETRIC = both(6, 8, {"bi_factor": 1.0, "width": 3.0}, {"bi_factor": 0.5, "width": 2.0})
# all of it on one network, for the cases about calls
MIXED = {**both(5, 6, {"length": 20.0, "fd_type": "greenshields", "speed_noise_std": 0.0}, {"length": 20.0, "fd_type": "greenshields", "speed_noise_std": 0.05}),
         **both(6, 7, {"fd_type": "smulders", "speed_noise_std": 0.0}, {"fd_type": "smulders", "speed_noise_std": 0.04}),
         **both(6, 8, {"length": 130.0, "bi_factor": 1.0, "width": 3.0}, {"length": 130.0, "bi_factor": 0.5, "width": 2.0, "speed_noise_std": 0.0}),
         **both(8, 9, {"length": 90.0, "free_flow_speed": 1.0, "k_jam": 5.0, "k_critical": 1.5}),
         **SAME_STEP_NOISE}
CASES = {"lengths": LENGTHS, "fd_types": FD_TYPES, "same_step_noise": SAME_STEP_NOISE, "asymmetric": ASYMMETRIC, "mixed": MIXED}


def start(R, links, knobs=None, env=None, oracle=True, dead=DEAD_LINKS):
    """The tree with `links`, the turn 1 -> 2 -> 5 closed and staggered demand at node 0.  env: set while BOTH engines are created."""
    adj, params, origins, dests = tree()
    params["links"] = {k: dict(v) for k, v in links.items()}
    keep = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        p = dl.Pair((adj, params, origins, dests), R, SEED, oracle=oracle, knobs=knobs)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    p.tf(2, 1, 5)
    p.demand(0, sd.staggered(p.T, R, key=3))
    assert p.dead() == dead
    return p


@pytest.mark.parametrize("R", [320, 330])
@pytest.mark.parametrize("case", sorted(CASES))
def test_records_that_differ_from_slot_to_slot(case, R):
    """One split range from t' = 1, in front of every free_flow_tau, shock-wave look-back and of W, to t' = 43, behind all of them.  330
    replicas leave a group with padding lanes."""
    p = start(R, CASES[case])
    p.run(1, 45)
    assert p.split_steps() == 43
    p.check(45, f"{case} x {R}")
    same = (p.on.error_flags()[1] & PEDN_F_SAME_STEP) != 0
    print(case, R, "replicas with the same-step flag:", int(same.sum()))
    if case in ("same_step_noise", "mixed"):
        assert same.any() and not same.all()   # raised by the dead link, per replica (check() has compared them: on, off, oracle)
    else:
        assert not same.any()
    assert p.dead() == DEAD_LINKS
    p.close()


def test_free_flow_travel_time_below_half_a_step():
    """The issue's case, a dead link with zero noise whose avg_travel_time / unit_time rounds to 0: see SAME_STEP above.  The flag is
    raised in every replica, the same on, off and in the oracle -- by the node kernel, because a link of free_flow_tau 0 invents
    pedestrians and nothing downstream of it is dead."""
    p = start(320, SAME_STEP, dead=0)
    p.run(1, 45)
    assert p.split_steps() == 0 and p.dead() == 0
    p.check(45, "free_flow_tau 0 at the dead end 8 - 11")
    flags = p.on.error_flags()[1]
    assert ((flags & PEDN_F_SAME_STEP) != 0).all()
    link = p.net.links[(8, 11)].index
    assert (p.on.read_block(ALL_FIELDS.index("sending_flow"), 0, 1, link, link + 1) == -1.0).all()      # what makes it a source
    p.close()


def test_shared_back_gate_set_to_another_valid_width_and_back():
    """After 15 steps of a split range the back gate of the dead link 6 -> 8 (width 3.0) becomes 2.0 in every replica: the link stays dead,
    its record is rebuilt, and the gate record is written from the next step on; then back to 3.0, which is not recorded."""
    p = start(320, MIXED)
    link = p.net.links[(6, 8)].index
    p.run(1, 17)
    assert p.split_steps() == 15
    p.width(1, link, 2.0)
    assert p.dead() == DEAD_LINKS
    p.run(17, 30)
    assert p.split_steps() == 15 + 12 and p.dead() == DEAD_LINKS
    p.check(30, "back gate 2.0 on the dead link 6 -> 8")
    rows = p.on.read_block(GATE, 0, 30, link, link + 1)
    assert (rows[17:29] == 2.0).all() and (rows[:16] == 3.0).all(), rows[:, 0, 0]
    p.width(1, link, 3.0)
    assert p.dead() == DEAD_LINKS
    p.run(30, 45)
    assert p.split_steps() == 15 + 12 + 14
    p.check(45, "back gate back at its own width")
    assert (p.on.read_block(GATE, 30, 45, link, link + 1) == 3.0).all()
    p.close()


def test_zero_elision_off():
    p = start(330, MIXED, env={"PEDN_ZERO_ELIDE": "0"})
    assert not p.on.plan_info()["zero_elide"] and not p.off.plan_info()["zero_elide"]
    p.run(1, 45)
    assert p.split_steps() == 43
    p.check(45, "PEDN_ZERO_ELIDE=0")
    p.close()


def test_two_lean_launches_per_step():
    p = start(330, MIXED, knobs={"PEDN_DEAD_STREAMS": "2"})
    p.run(1, 45)
    assert p.split_steps() == 43
    p.check(45, "PEDN_DEAD_STREAMS=2")
    p.close()


def test_lazy_reset_in_the_middle_of_a_split_range():
    p = start(320, MIXED)
    p.run(1, 20)
    assert p.split_steps() == 18
    p.reset(lazy=True)
    assert p.dead() == DEAD_LINKS              # the same sources: nothing to narrow
    p.run(1, 12)
    p.run(12, 40)
    assert p.split_steps() == 10 + 27
    p.check(40, "second episode after a lazy reset")
    p.close()


def test_full_reset_then_a_range_that_is_split_again():
    p = start(320, MIXED)
    p.run(1, 20)
    assert p.split_steps() == 18
    p.reset()
    assert p.dead() == DEAD_LINKS
    p.run(1, 30)
    assert p.split_steps() == 28               # counted from the reset; the first node launch of a range stays on the full bin set
    p.check(30, "second episode after a full reset")
    p.close()


def test_melbourne_as_the_benchmark_builds_it():
    """melbourne x 256 with the benchmark's demand, 30 steps: the plan on against off by bits (the oracle: test_gpu_dead_links.py)."""
    from golden_util import DATA
    from pednstream_amd import NetworkEnvGenerator
    from test_gpu_quiet_corridors import poisson_demand

    R, steps = 256, 30
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
        got, want = on.read_block(fid, 0, steps), off.read_block(fid, 0, steps)
        word = np.uint64 if got.dtype.itemsize == 8 else np.uint32
        if not np.array_equal(got.view(word), want.view(word)):          # (one pass over 80 MB; the slower comparison names the entry)
            assert_same_bits(got, want, f"melbourne x {R}: {name}", "[t, column, replica]")
    assert on.read_block(2, steps - 1, steps).sum() > 0          # somebody walks
    for net, _ in engines:
        net.close()
