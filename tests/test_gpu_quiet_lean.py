"""Lean quiet step (PEDN_QUIET_LEAN): in the quiet-corridor launches of node_kernel<LU>, a slot wave whose products P[slot][j] * s_slot are
+0.0 in all 64 lanes skips its row sums, and one whose column of products is +0.0 in all 64 lanes skips its column pass; link_flow
joins the zero-elided fields.  Every case builds the same engine twice -- PEDN_QUIET_LEAN=1 and =0, read by pedn_create -- drives both
through the same calls and asks for identical bits in every history field (all rows, columns and replicas, straight from device
memory), the error flags and the turning fractions."""
import copy
import os

import numpy as np
import pytest

from fuzz_cases import random_case
from golden_util import DATA
from pednstream_amd import Network, NetworkEnvGenerator
from test_gpu_quiet_corridors import assert_same, poisson_demand

pytestmark = pytest.mark.gpu

KEYS = ("PEDN_QUIET_LEAN", "PEDN_STREAMS", "PEDN_STREAM_PROBE")


def make(build, on, env=None):
    """build() -> a network whose engine is created with PEDN_QUIET_LEAN=on and `env` set (pedn_create reads them once)"""
    keep = {k: os.environ.get(k) for k in KEYS}
    os.environ["PEDN_QUIET_LEAN"] = "1" if on else "0"
    os.environ.update(env or {})
    try:
        net = build()
        net.engine()
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return net


def set_demand(net, scale, key=0):
    T, R = net.simulation_steps, net.engine().n_replicas
    for nid in net.origin_nodes:
        net.set_demand_matrix(nid, np.stack([poisson_demand(T, 31 * r + nid + key, scale) for r in range(R)]))


def model(name, R, scale=1.0, env=None, history="full"):
    def build():
        np.random.seed(7)
        net = NetworkEnvGenerator(DATA).create_network(name, verbose=False, n_replicas=R, rng_seed=5, history=history)
        net.engine()
        if scale is not None:
            set_demand(net, scale)
        return net
    return make(build, True, env), make(build, False, env)


def lean(net):
    return net.engine().plan_info()["quiet_lean"]


def test_the_setting_is_reported():
    a, b = model("melbourne", 64)
    assert lean(a) and not lean(b)
    a.close(), b.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_headline_full_horizon(streams):
    """melbourne x 1024 with bench.py's demand over the whole horizon (longer than the travel-time window W), one and two chains"""
    a, b = model("melbourne", 1024, env={"PEDN_STREAMS": str(streams), "PEDN_STREAM_PROBE": "0"})
    assert lean(a) and a.engine().plan_info()["chains"] == streams
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, f"melbourne x 1024, {streams} chain(s)")
    a.close(), b.close()


def test_heavy_demand():
    a, b = model("melbourne", 1024, scale=12.0)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, "melbourne x 1024, demand x 12")
    a.close(), b.close()


@pytest.mark.parametrize("name,R", [("delft", 256), ("45_intersections", 512)])
def test_other_models(name, R):
    a, b = model(name, R)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, name)
    a.close(), b.close()


def test_separators():
    """a random network with four separators, two chains of 256 replicas"""
    adj, params, origins, dests = random_case(15)
    assert sum(v.get("controller_type") == "separator" for v in params["links"].values()) == 4

    def build():
        np.random.seed(15)
        return Network(adj, copy.deepcopy(params), origin_nodes=origins, destination_nodes=dests, verbose=False, n_replicas=256, rng_seed=15)

    env = {"PEDN_STREAMS": "2", "PEDN_STREAM_PROBE": "0"}
    a, b = make(build, True, env), make(build, False, env)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, "separators")
    a.close(), b.close()


def test_short_links():
    """corridors shorter than half a time step: look-backs of zero steps into the row this launch writes"""
    adj, params, origins, dests = random_case(21, short_links=True)

    def build():
        np.random.seed(21)
        return Network(adj, copy.deepcopy(params), origin_nodes=origins, destination_nodes=dests, verbose=False, n_replicas=256, rng_seed=21)

    a, b = make(build, True), make(build, False)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, "short links")
    a.close(), b.close()


def test_gates_set_between_steps():
    a, b = model("melbourne", 256, scale=3.0)
    T = a.simulation_steps
    for n in (a, b):
        e = n.engine()
        for t in range(1, min(T, 160)):
            e.step(t)
            if t % 23 == 0:
                e.set_width(0, 5, 1.5 + 0.01 * t)     # front gate of link 5, every replica
            if t % 31 == 0:
                e.set_width(1, 7, 0.0)                # back gate of link 7 closed
        e.run(min(T, 160), T)
    assert_same(a, b, "gates set between steps")
    a.close(), b.close()


def test_lazy_reset_then_a_second_episode():
    a, b = model("melbourne", 512, scale=12.0)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
        n.engine().reset(lazy=True)
        set_demand(n, 0.5, key=7)
        n.engine().run(1, T)
    assert_same(a, b, "lazy reset, then a second episode")
    a.close(), b.close()


def test_recent_history():
    a, b = model("melbourne", 256, scale=3.0, history="recent")
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, "recent-history mode")
    a.close(), b.close()
