"""The host proof behind the dead-link plan (pednstream_amd/csrc/pedn_partition.hpp), without a GPU: its stand-alone driver built with
AddressSanitizer + UBSan runs the hand-made models, and on the flattened model of every network under data/ the C++ answer equals the
propagation rules restated in Python (tests/partition_model.py)."""
import os
import subprocess

import numpy as np
import pytest

import partition_model as pm
from golden_util import DATA
from pednstream_amd import NetworkEnvGenerator
from pednstream_amd.flatten import flatten_network

NETWORKS = sorted(d for d in os.listdir(DATA) if os.path.isdir(os.path.join(DATA, d)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return pm.build_prog(tmp_path_factory.mktemp("partition"))


def test_hand_made_models_under_the_sanitizers(prog):
    r = subprocess.run([prog, "selftest"], capture_output=True, text=True)
    assert r.returncode == 0 and "selftest ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", NETWORKS)
def test_library_answer_equals_the_python_restatement(prog, name, tmp_path):
    np.random.seed(0)
    net = NetworkEnvGenerator(DATA).create_network(name, verbose=False)
    inp = pm.proof_inputs(flatten_network(net))
    mine = pm.partition(inp)
    lib = pm.run_prog(prog, inp, tmp_path / "model.txt")
    for key in ("reach", "live", "dead_raw", "node_dead", "dead"):
        assert lib[key] == mine[key], (name, key, sorted(lib[key] ^ mine[key])[:10])
    print(name, {k: len(v) for k, v in mine.items()})
    if name == "melbourne":
        assert mine["reach"] == {15, 18, 23, 317, 856, 880, 914}
        assert len(mine["live"]) == 8
        # closed branch with an open twin: the same model with per-replica OD weights (every tabulated turn possible) keeps less
        inp2 = dict(inp, tab_nz=np.ones_like(inp["tab_nz"]))
        assert pm.run_prog(prog, inp2, tmp_path / "model2.txt")["dead"] <= lib["dead"]
