"""The host model of the reference's evaluation metrics (tests/metrics_model.py) against the values the reference's own
rl/rl_utils.py returned for the same runs (tests/golden/metrics_<case>.json, tools/gen_metric_goldens.py): bit for bit.  The
output_* cases feed it the JSON the reference's OutputHandler wrote; the others the CPU oracle's histories.  Plus the pieces of
pednstream_amd.metrics that need no GPU."""
import json
import os
import zlib

import numpy as np
import pytest

import metrics_model as mm
from golden_util import GOLDEN, Golden, run_oracle

JSON_CASES = ["output_six_node", "output_corridor"]
ORACLE_CASES = ["six_node_full", "butterfly_scA_full", "i45_full", "delft_full", "melbourne_full"]
# the same runs continued through t = T (row T: the cumulative flows throughput and served-trip rate read)
THROUGH_T_CASES = ["six_node_full_through_T", "delft_full_through_T"]


def fixture(case):
    with open(os.path.join(GOLDEN, f"metrics_{case}.json")) as f:
        return json.load(f)["metrics"]


def ref_json(g, name):
    return json.loads(zlib.decompress(g.z["json_" + name].tobytes()).decode())


def agent_keys(net):
    from pednstream_amd.metrics import agent_links

    ids, ptr, _, keys = agent_links(net)
    return {aid: keys[ptr[a]:ptr[a + 1]] for a, aid in enumerate(ids)}


def check(link_data, node_data, params, want, net=None):
    got = json.loads(json.dumps(mm.reference_metrics(link_data, node_data, params)))
    for name in mm.NAMES:
        assert got[name] == want[name], (name, got[name], want[name])
    if "agent_local_metrics" in want:
        ag = json.loads(json.dumps(mm.agent_local_metrics(link_data, agent_keys(net))))
        assert ag == want["agent_local_metrics"]


@pytest.mark.parametrize("case", JSON_CASES)
def test_model_on_reference_json_equals_reference(case):
    g = Golden(case)
    want = fixture(case)
    net = None
    if "agent_local_metrics" in want:
        from golden_util import build_network

        net = build_network(g)
    check(ref_json(g, "link_data"), ref_json(g, "node_data"), ref_json(g, "network_params"), want, net)


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_model_on_oracle_histories_equals_reference(case):
    g = Golden(case)
    o, _, _, net = run_oracle(g)
    check(mm.link_data_from(net, o.field), mm.node_data_from(net), mm.params_from(net), fixture(case), net)


@pytest.mark.parametrize("case", THROUGH_T_CASES)
def test_model_through_row_T_equals_reference(case):
    g = Golden(case[:-len("_through_T")])
    o, _, _, net = run_oracle(g)
    o.step(net.simulation_steps)
    want = fixture(case)
    assert want["served_trips_rate"]["total_outflow"] > 0 and want["network_throughput"]["throughput"] > 0
    check(mm.link_data_from(net, o.field), mm.node_data_from(net), mm.params_from(net), want, net)


def test_fixtures_are_small_and_cover_every_metric():
    for case in JSON_CASES + ORACLE_CASES + THROUGH_T_CASES:
        path = os.path.join(GOLDEN, f"metrics_{case}.json")
        assert os.path.getsize(path) < 64 * 1024
        want = fixture(case)
        assert set(mm.NAMES) <= set(want)
    assert any("agent_local_metrics" in fixture(c) for c in JSON_CASES + ORACLE_CASES)


def test_link_flags_and_agent_links():
    """The static set-up pedn_metrics_begin receives: origin / destination / od-path bits, and the agents' links."""
    from golden_util import build_network
    from pednstream_amd.metrics import agent_links, link_flags

    net = build_network(Golden("six_node_full"))
    flags = link_flags(net)
    for (u, v), link in net.links.items():
        assert bool(flags[link.index] & 1) == (u in net.origin_nodes)
        assert bool(flags[link.index] & 2) == (v in net.destination_nodes)
    assert (flags & 4).any() and not (flags & 4).all()        # od paths select a subset here
    net = build_network(Golden("output_corridor"))
    ids, ptr, links, keys = agent_links(net)
    assert ids == ["sep_2_3"] and list(ptr) == [0, 2] and keys == ["2-3", "3-2"]


def test_replica_gives_plain_reference_dicts():
    from pednstream_amd.metrics import LAYOUT, _dicts, replica

    out = np.arange(2 * 23, dtype=np.float64).reshape(2, 23)
    res = _dicts(out)
    assert set(res) == set(LAYOUT) and res["network_congestion"]["counted_rows"].dtype == np.int64
    one = replica(res, 1)
    assert list(one["network_throughput"]) == ["throughput", "completed_demand", "total_demand", "completion_rate"]
    assert one["network_throughput"]["throughput"] == 23.0 and one["network_throughput"]["completion_rate"] == 23.0
    assert one["served_trips_rate"]["num_origin_links"] == 35 and isinstance(one["served_trips_rate"]["num_origin_links"], int)
    assert "counted_rows" not in one["network_congestion"]
