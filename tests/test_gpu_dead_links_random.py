"""The dead-link plan of pedn_run on random networks under random sequences of calls: the engine with PEDN_DEAD_LINKS=1 against the same
engine with PEDN_DEAD_LINKS=0 against the CPU oracle, by bits, and the engine's bookkeeping of the proof's inputs against a copy the
test keeps itself (dead_link_cases.Proof: the Python restatement of the proof on inputs updated call by call).

A case is fuzz_cases.random_case(seed) with the closed turns, zero demand rows and sparse OD weights of dead_link_cases.mutate, sparse
demand (sparse_demand.staggered) in every origin row that is left, 320 or 330 replicas on two chains, and dead_link_cases.call_sequence:
10 to 16 calls -- ranges and single steps, turns opened and closed, fractions of one replica, uploads into zero rows by all three demand
calls, a row zeroed, gates on dead and live links (0.0, 0.5, -1.0, inf, NaN; the oracles leave at the last two), reads and flushes in
mid-run, lazy and full resets.  Position i of the list makes sure of two kinds of call, so that the list as a whole has every kind.
After every call plan_info() must give the dead-link count and the lean-kernel steps the test's own copy gives; at two checkpoints and
at the end every field, row, column and replica and the flags are compared.

CASES is chosen on the CPU (no row of fractions computed on the device, at least 2 dead and 2 reached links, the sampled oracle replicas
free of flags over the horizon); tests/test_partition_soundness.py recomputes every figure in it without a GPU."""
import pytest

import dead_link_cases as dl

pytestmark = pytest.mark.gpu

# seed, replicas, how the mutation reaches the engines (dead_link_cases.start), nodes, T, |REACH|, dead links before eligibility, dead links,
# host-tabulated rows (an OD model), calls, and after the last call: dead links, lean-kernel steps since the last reset
CASES = (
    (4017, 320, "create", 13, 139, 5, 20, 7, 1, 15, 0, 82),
    (4020, 320, "setters", 8, 152, 4, 5, 5, 0, 10, 5, 14),
    (4026, 330, "create", 9, 136, 2, 10, 10, 0, 12, 2, 65),
    (4027, 320, "setters", 11, 135, 8, 10, 10, 0, 16, 0, 18),
    (4055, 320, "create", 10, 125, 4, 7, 4, 1, 11, 1, 16),
    (4067, 320, "setters", 11, 148, 6, 10, 10, 1, 11, 1, 32),
    (4072, 320, "create", 13, 139, 2, 24, 19, 1, 13, 19, 82),
    (4093, 320, "setters", 13, 85, 7, 9, 4, 0, 15, 3, 11),
    (4098, 330, "create", 8, 156, 8, 6, 3, 1, 15, 0, 0),
    (4120, 320, "setters", 9, 152, 2, 11, 6, 0, 15, 0, 21),
    (4125, 320, "create", 8, 105, 3, 7, 7, 1, 10, 0, 20),
    (4161, 330, "setters", 13, 114, 4, 20, 20, 1, 15, 11, 23),
    (4321, 320, "create", 13, 110, 2, 24, 17, 1, 15, 10, 19),
    (4275, 320, "setters", 10, 86, 3, 14, 13, 1, 14, 11, 48),
)


# What the campaign tools/gpu_fuzz_dead_links.py found (seeds 4000..5000, three of 314 networks with PEDN_DEAD_LINKS=1 differing from
# PEDN_DEAD_LINKS=0), with the two kinds of call each was drawn with.  4230 and 4566: a front gate of -1.0 in one replica, on a link in
# front of a one-to-one node -- the link sends a negative flow, the node hands it on, and the link behind the node was still stepped
# as dead.  4481: an origin's row zeroed while its pedestrians were walking, then a turn opened in front of them -- the proof, run
# afresh without a source, kept the branch behind that turn dead.  (Two of them have no demand at all, so they are not part of CASES.)
REGRESSIONS = (
    ((4230, 320, "create", 6, 130, 0, 10, 10, 0, 11, 3, 23), ("tf_one_replica", "gate_one_replica")),
    ((4481, 320, "setters", 9, 136, 7, 3, 3, 0, 15, 3, 42), ("close_turn", "gate_live")),
    ((4566, 320, "create", 12, 128, 0, 22, 22, 1, 14, 1, 15), ("tf_one_replica", "gate_one_replica")),
)


def must(i):
    """the two kinds of call that position i of CASES is sure to make"""
    n = len(dl.KINDS)
    return dl.KINDS[i % n], dl.KINDS[(i + n // 2) % n]


EVERY = tuple((row, must(i)) for i, row in enumerate(CASES)) + REGRESSIONS


def test_most_cases_end_on_the_split_plan():
    """13 of the 14: in the other one the calls have made every node live by then"""
    assert len(CASES) >= 12 and 12 * sum(c[11] > 0 for c in CASES) >= 10 * len(CASES)
    assert sum(c[1] == 330 for c in CASES) == 3


@pytest.mark.parametrize("row,kinds", EVERY, ids=[str(row[0]) for row, _ in EVERY])
def test_random_network_under_random_calls(row, kinds):
    seed, R, mode, _, _, _, _, dead0, _, _, dead1, split1 = row
    case, m, rec = dl.mutated_case(seed)
    calls, expect = dl.call_sequence(m, R, seed, kinds)
    p = dl.start(case, m, rec, R, seed, mode)
    assert p.dead() == dead0 and p.split_steps() == 0
    dl.run_calls(p, calls, expect, f"seed {seed} x {R}")
    assert (p.dead(), p.split_steps()) == (dead1, split1) == expect[-1][:2]
    p.close()
