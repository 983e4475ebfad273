"""The planner that the CPU test checks (tests/test_step_plan_host.py) is the one the library steps with: one fixed session of 20 steps --
pedn_reset, pedn_run(1, 10), a pedn_read, three consecutive pedn_step calls, pedn_run(13, 21) -- goes through the library and, as the events
plan_model.session_events makes of it, through the stand-alone driver tests/plan_prog.cpp under the caps that the driver's own plan chooser
gives for the model's compiled facts (tests/compile_prog.cpp) and the knob; what the library reports of its plan (pedn_plan_info entries 1, 5,
6, 8) must be that plan's report.  The launches with a zero gate open (info[7]) and the split steps (info[10]) the library counts must be the
planner's.  Two chains are asked for (256 replicas would step as one); whether they and the split plan are taken depends on the machine's
stream probe, and the prediction follows what the library reports."""
import os

import numpy as np
import pytest

import compile_model as cm
import dead_link_cases as dl
import partition_model as part
import plan_model as pm
from golden_util import DATA

pytestmark = pytest.mark.gpu

R = 256
CALLS = (("reset",), ("run", 1, 10), ("read",), ("step", 10), ("step", 11), ("step", 12), ("run", 13, 21))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return pm.build_prog(tmp_path_factory.mktemp("plan"))


@pytest.fixture(scope="module")
def compiler(tmp_path_factory):
    return cm.build_prog(tmp_path_factory.mktemp("compile"))


def corridor():
    from pednstream_amd import NetworkEnvGenerator
    from pednstream_amd.flatten import flatten_network

    np.random.seed(7)
    net = NetworkEnvGenerator(DATA).create_network("long_corridor", verbose=False, n_replicas=R, rng_seed=11)
    return net, net.engine(), flatten_network(net)


def dead_network():
    """a random network whose mutated model has 10 dead links and no host-tabulated row (tests/test_gpu_dead_links_random.py, seed 4026)"""
    from pednstream_amd.engine import Engine

    _, m, _ = dl.mutated_case(4026)
    return None, Engine(m, n_replicas=R, seed=4026), m


@pytest.mark.parametrize("make", (corridor, dead_network), ids=("long_corridor", "dead_links"))
def test_the_library_counts_what_the_planner_plans(prog, compiler, make, tmp_path):
    keep = os.environ.get("PEDN_STREAMS")
    os.environ["PEDN_STREAMS"] = "2"          # read when the engine is created
    try:
        net, e, model = make()
    finally:
        os.environ.pop("PEDN_STREAMS", None) if keep is None else os.environ.__setitem__("PEDN_STREAMS", keep)
    assert not (np.asarray(part.proof_inputs(model)["slot_dyn"]) == 1).any()          # no row of fractions computed on the device
    assert e.n_replicas == R and int(model["T"]) >= 21 and int(model.get("history_mode", 0)) == 0          # full histories
    info = e.plan_info()
    if make is dead_network:
        assert info["dead_links"] in (0, 10)          # 0: no two chains, or no third stream that overlaps with them
    cm.write_model(model, tmp_path / "model.txt")
    inputs, _ = pm.compiled_inputs(cm.run_prog(compiler, tmp_path / "model.txt", R), model, R)
    plan = pm.choose_one(prog, inputs, pm.knobs_of(dict(os.environ, PEDN_STREAMS="2")), tmp_path / "choose.txt")
    assert (info["link_update_by_next_node_kernel"], info["quiet_corridors"], info["zero_elide"], info["quiet_lean"]) == \
        (plan["r_owner_wave"], plan["r_quiet"], plan["r_zero_elide"], plan["r_quiet_lean"]) and info["chains"] <= plan["chains"] == 2
    caps = pm.caps_of(plan, rl_ready=0, pr=0, trow=int(inputs["n_trow"] > 0), links=inputs["links"], live=1, T1=int(model["T"]) + 1)
    lean = 2 if os.environ.get("PEDN_DEAD_STREAMS", "1") != "1" else 1
    events = pm.session_events(info["chains"], info["link_update_by_next_node_kernel"], info["dead_links"], CALLS, lean=lean, rs=(R + 127) // 128 * 128)
    result = pm.run_prog(prog, [(caps, events)], tmp_path / "session.txt")[0]
    planned = result[-1][1]
    for call in CALLS:
        if call[0] == "reset":
            e.reset()
        elif call[0] == "run":
            e.run(call[1], call[2])
        elif call[0] == "step":
            e.step(call[1])
        else:
            e.read_block(2, 9, 10, rep0=0, rep1=1)
    after = e.plan_info()
    print(make.__name__, info, "gated launches", after["zero_elide_launches"], "split steps", after["dead_link_steps"], "planned", planned)
    assert (after["zero_elide_launches"], after["dead_link_steps"]) == (planned["zgated"], planned["split_steps"])
    assert planned["last_t"] == 20 and planned["split_steps"] == (15 if info["dead_links"] else 0)
    e.synchronize()
    (net.close if net is not None else e.close)()
