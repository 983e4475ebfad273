"""The plan chooser that the CPU test checks (tests/test_step_plan_host.py) is the one pedn_create chooses with: at the smallest shapes that
reach each branch an engine is created under a set of PEDN_* knobs, and its pedn_plan_info must be what the stand-alone driver
(tests/plan_prog.cpp --choose) reports for the same inputs -- the compiled facts of the model from tests/compile_prog.cpp and the knobs.
Entries 1, 4, 5, 6 and 8 are equal; entry 0 is at most the chains wanted (the stream probe may take it down); entry 9 is 0 or the proof's
count.  Then ten steps under that plan read back bit for bit what the default plan is pinned to: the reference's golden of the scenario
(golden_util.compare_fields), and for the generated dead-link network, which has none, an engine of the same model under the default plan."""
import os

import numpy as np
import pytest

import compile_model as cm
import dead_link_cases as dl
import plan_model as pm
from golden_util import ALL_FIELDS, Golden, build_network, compare_fields
from pednstream_amd.flatten import flatten_network
from pednstream_amd.network import LINK_FIELDS

pytestmark = pytest.mark.gpu

STEPS = 10
PACKED_BY = ("degree", "static_load_estimate", "measured_node_cost")
# (golden or None: the dead-link network of tests/test_gpu_step_plan.py, replicas, knobs, what the branch is -- checked on the driver's plan)
CASES = {
    "owner_wave_one_chain": ("long_corridor_full", 128, {}, dict(link_owner=1, inline_tf=0, quiet=1, chains=1)),
    "single_launch_helpers": ("nine_full", 256, {}, dict(link_owner=1, inline_tf=1, inline_help=1, chains=1)),
    "two_launches": ("nine_full", 256, {"PEDN_INLINE_TF": "0"}, dict(link_owner=0, inline_tf=0, quiet=0)),
    "single_launch_own_rows": ("nine_full", 256, {"PEDN_INLINE_TF": "1"}, dict(link_owner=1, inline_tf=1, inline_help=0)),
    "no_owner_waves_no_words": ("long_corridor_full", 128, {"PEDN_LINK_OWNER": "0", "PEDN_QUIET": "0"}, dict(link_owner=0, quiet=0, dead_capable=0)),
    "dead_links_two_chains": (None, 256, {"PEDN_STREAMS": "2"}, dict(link_owner=1, quiet=1, chains=2, dead_capable=1)),
}
KNOB_NAMES = tuple("PEDN_" + k.upper() for k in pm.KNOBS)


@pytest.fixture(scope="module")
def progs(tmp_path_factory):
    d = tmp_path_factory.mktemp("engine_plan")
    return pm.build_prog(d), cm.build_prog(d)


def create(golden, replicas, knobs):
    """(network or None, engine, flattened model) created with exactly `knobs` of the step-plan knobs in the environment"""
    keep = {k: os.environ.pop(k) for k in KNOB_NAMES if k in os.environ}
    os.environ.update(knobs)          # read when the engine is created
    try:
        if golden is None:
            from pednstream_amd.engine import Engine

            _, m, _ = dl.mutated_case(4026)          # 10 dead links, no host-tabulated row (tests/test_gpu_dead_links_random.py)
            return None, Engine(m, n_replicas=replicas, seed=4026), m
        g = Golden(golden)
        net = build_network(g, n_replicas=replicas, replica_offset=g.replica, rng_seed=g.seed, rng_mode=g.mode)
        return net, net.engine(), flatten_network(net)
    finally:
        for k in knobs:
            os.environ.pop(k, None)
        os.environ.update(keep)


def fields_after_run(e, rep1):
    e.run(1, STEPS + 1)
    out = {name: e.read_block(LINK_FIELDS[name][0], 0, STEPS + 1, rep0=0, rep1=rep1) for name in ALL_FIELDS}          # [t, columns, replicas]
    assert e.error_flags()[0] == 0
    return out


@pytest.fixture(scope="module")
def dead_network_default():
    """the dead-link network under the default plan: every field, every replica, once"""
    net, e, _ = create(None, 256, {})
    out = fields_after_run(e, 256)
    e.close()
    return out


@pytest.mark.parametrize("case", CASES)
def test_the_library_chooses_what_the_driver_chooses(progs, case, tmp_path, request):
    planner, compiler = progs
    golden, replicas, knobs, branch = CASES[case]
    net, e, model = create(golden, replicas, knobs)
    cm.write_model(model, tmp_path / "model.txt")
    inputs, packed_by = pm.compiled_inputs(cm.run_prog(compiler, tmp_path / "model.txt", replicas), model, replicas)
    plan = pm.choose_one(planner, inputs, pm.knobs_of(knobs), tmp_path / "choose.txt")
    assert {k: plan[k] for k in branch} == branch, plan          # the case reaches the branch it is here for
    info = e.plan_info()
    print(case, info, {k: v for k, v in plan.items() if not k.startswith("k_")})
    assert info["link_update_by_next_node_kernel"] == plan["r_owner_wave"] and info["packed_by"] == PACKED_BY[packed_by]
    assert (info["quiet_corridors"], info["zero_elide"], info["quiet_lean"]) == (plan["r_quiet"], plan["r_zero_elide"], plan["r_quiet_lean"])
    assert 1 <= info["chains"] <= plan["chains"]
    proof = 10 if golden is None else None          # (the scenarios' engines step on one chain: no split)
    assert info["dead_links"] == 0 or (plan["r_dead_links"] and info["chains"] == 2 and info["dead_links"] == proof), info
    if golden is None:
        want = request.getfixturevalue("dead_network_default")
        got = fields_after_run(e, replicas)
        assert e.plan_info()["dead_link_steps"] == (STEPS - 1 if info["dead_links"] else 0)
        for name in ALL_FIELDS:
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name
    else:
        got = fields_after_run(e, 1)
        g = Golden(golden)
        problems = compare_fields(lambda name: got[name][:, :, 0].T, g, e.n_links, STEPS)
        assert not problems, "\n".join(problems)
        for name in ALL_FIELDS:          # ... and row STEPS of what step STEPS writes there (its sending / receiving flows are entries STEPS - 1)
            if name not in ("sending_flow", "receiving_flow"):
                assert np.array_equal(got[name][STEPS, :e.n_links, 0], g.state(name)[:, STEPS]), name
    (net.close if net is not None else e.close)()
