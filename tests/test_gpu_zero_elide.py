"""Zero elision (PEDN_ZERO_ELIDE): a node-kernel wave skips a pair of history stores whose values are +0.0 in all 64 lanes when the host
vouches that the row holds +0.0 since the last full reset.  Every case builds the same engine twice -- PEDN_ZERO_ELIDE=1 and =0, read
by pedn_create -- drives both through the same calls and asks for identical bits in every history field (all rows, columns and
replicas, straight from device memory), the error flags and the turning fractions.  plan_info()["zero_elide_launches"] (node-kernel
launches with a gate open since the last reset) shows that the skipping path really ran -- or, on dirty rows, that it did not."""
import copy
import os

import numpy as np
import pytest

from fuzz_cases import random_case
from golden_util import DATA
from pednstream_amd import Network, NetworkEnvGenerator
from test_gpu_quiet_corridors import assert_same, poisson_demand

pytestmark = pytest.mark.gpu

KEYS = ("PEDN_ZERO_ELIDE", "PEDN_STREAMS", "PEDN_LINK_OWNER", "PEDN_STREAM_PROBE")


def make(build, on, env=None):
    """build() -> a network whose engine is created with PEDN_ZERO_ELIDE=on and `env` set (pedn_create reads them once)"""
    keep = {k: os.environ.get(k) for k in KEYS}
    os.environ["PEDN_ZERO_ELIDE"] = "1" if on else "0"
    os.environ.update(env or {})
    try:
        net = build()
        net.engine()
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert net.engine().plan_info()["zero_elide"] == on
    return net


def set_demand(net, scale, key=0):
    T, R = net.simulation_steps, net.engine().n_replicas
    for nid in net.origin_nodes:
        net.set_demand_matrix(nid, np.stack([poisson_demand(T, 31 * r + nid + key, scale) for r in range(R)]))


def model(name, R, scale=1.0, env=None):
    def build():
        np.random.seed(7)
        net = NetworkEnvGenerator(DATA).create_network(name, verbose=False, n_replicas=R, rng_seed=5)
        net.engine()
        if scale is not None:
            set_demand(net, scale)
        return net
    return make(build, True, env), make(build, False, env)


def gated(net):
    return net.engine().plan_info()["zero_elide_launches"]


@pytest.mark.parametrize("streams", [1, 2])
def test_forward_run_headline(streams):
    """melbourne x 1024 with bench.py's demand, one range over the horizon: the gates open, the bits are those of the full stores"""
    a, b = model("melbourne", 1024, env={"PEDN_STREAMS": str(streams)})
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert gated(a) >= T - 1 and gated(b) == 0, (gated(a), gated(b))
    assert_same(a, b, f"melbourne x 1024, {streams} chain(s)")
    a.close(), b.close()


def test_busy_corridors():
    """melbourne heavy (x 12 demand): many waves with some lanes non-zero -- a wave stores the whole row segment or none of it"""
    a, b = model("melbourne", 1024, scale=12.0)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert gated(a) > 0
    assert_same(a, b, "melbourne x 1024, demand x 12")
    a.close(), b.close()


@pytest.mark.parametrize("name", ["delft", "melbourne_two_launch"])
def test_two_launch_plan(name):
    """the plain node kernel of the two-launch plan: delft, and melbourne with the owner-wave link update turned off"""
    env = {"PEDN_LINK_OWNER": "0"} if name == "melbourne_two_launch" else None
    a, b = model(name.split("_")[0], 256, env=env)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert gated(a) > 0
    assert_same(a, b, name)
    a.close(), b.close()


def test_separators():
    """a random network with four separators (its density is not num_pedestrians / area), two chains of 256 replicas"""
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
    assert gated(a) > 0
    assert_same(a, b, "separators")
    a.close(), b.close()


def test_reads_and_flushes_between_steps():
    a, b = model("melbourne", 256, scale=3.0)
    T = a.simulation_steps
    for n in (a, b):
        e = n.engine()
        for t in range(1, min(T, 120)):
            e.step(t)
            if t % 13 == 0:
                e.read_block(9, t - 1, t)
            if t % 19 == 0:
                e.flush()
        e.run(min(T, 120), T)
    assert gated(a) > 0
    assert_same(a, b, "reads and flushes between steps")
    a.close(), b.close()


def test_repeated_and_jumping_steps():
    """a step run again (its rows were written: no gate), and steps that jump ahead after a lazy reset"""
    a, b = model("melbourne", 256, scale=4.0)
    T = a.simulation_steps
    for n in (a, b):
        e = n.engine()
        e.run(1, 40)
        e.step(39)
        e.step(39)
        e.run(40, 60)
        e.reset(lazy=True)
        e.step(1)
        e.step(25)
        e.run(26, 50)
        e.step(80)
        e.run(81, T)
    assert_same(a, b, "repeated and jumping steps")
    a.close(), b.close()


def test_lazy_reset_then_a_quieter_episode():
    """a heavy episode to the end of the horizon, a lazy reset, then a light one: corridors that were busy are quiet now, and the rows
    they skip would still hold the heavy episode's values -- no gate may open on them"""
    a, b = model("melbourne", 512, scale=12.0)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert gated(a) > 0
    for n in (a, b):
        n.engine().reset(lazy=True)
        set_demand(n, 0.5, key=7)
        n.engine().run(1, T)
    assert gated(a) == 0
    assert_same(a, b, "lazy reset, then a quieter episode")
    a.close(), b.close()


def test_full_reset_reopens_the_gates():
    a, b = model("melbourne", 512, scale=12.0)
    T = a.simulation_steps
    for n in (a, b):
        e = n.engine()
        e.run(1, T)
        e.reset()
        set_demand(n, 0.5, key=7)
        e.run(1, T)
    assert gated(a) >= T - 1
    assert_same(a, b, "full reset after a dirty episode")
    a.close(), b.close()


def test_zero_copy_pointer_closes_the_gates():
    """after pedn_device_ptr on the flows and on num_pedestrians a consumer may write any row: no gate until the next full reset"""
    a, b = model("melbourne", 256)
    T = a.simulation_steps
    for n in (a, b):
        e = n.engine()
        e.run(1, 30)
        assert e.device_ptr(0)[0] and e.device_ptr(9)[0]   # inflow, num_pedestrians
        before = gated(n)
        e.run(30, T)
        assert gated(n) == before
    assert gated(a) > 0
    for n in (a, b):
        n.engine().reset()
        n.engine().run(1, 30)
    assert gated(a) > 0
    assert_same(a, b, "zero-copy pointer")
    a.close(), b.close()
