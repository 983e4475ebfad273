"""Quiet corridors (node_kernel<LU>, PEDN_QUIET): a slot wave whose corridor was empty in all 64 replicas of its group at the last
step skips the loads the zero state determines and runs the same code on +0.0.  Every case here builds the same engine twice --
PEDN_QUIET=1 and PEDN_QUIET=0, read by pedn_create -- drives both through the same calls and asks for identical bits in every history
field (all rows, all columns, all replicas, straight from device memory), the error flags and the turning fractions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from golden_util import DATA
from pednstream_amd import NetworkEnvGenerator

pytestmark = pytest.mark.gpu

N_FIELDS = 13


def poisson_demand(T, key, scale=1.0):
    """bench.py's per-replica origin demand (replica_demand), times `scale`"""
    t = np.arange(T)
    base, peak = 5.0 * scale, 10.0 * scale
    lam = base + peak * np.exp(-(t - T / 4) ** 2 / (2 * (T / 20) ** 2)) + peak * np.exp(-(t - 3 * T / 4) ** 2 / (2 * (T / 20) ** 2))
    return np.random.default_rng(1000 + key).poisson(lam).astype(np.float64)


def make(name, R, quiet, streams=None, demand=None):
    """(net, engine) with PEDN_QUIET / PEDN_STREAMS set while the engine is CREATED (pedn_create reads them once; create_network
    does not create the engine, net.engine() does); demand(T, key, r) -> the row of replica r, or None"""
    keep = {k: os.environ.get(k) for k in ("PEDN_QUIET", "PEDN_STREAMS")}
    os.environ["PEDN_QUIET"] = "1" if quiet else "0"
    if streams is not None:
        os.environ["PEDN_STREAMS"] = str(streams)
    try:
        np.random.seed(7)
        net = NetworkEnvGenerator(DATA).create_network(name, verbose=False, n_replicas=R, rng_seed=5)
        e = net.engine()
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    info = e.plan_info()
    assert info["link_update_by_next_node_kernel"], info
    assert info["quiet_corridors"] == quiet, (quiet, info)       # the setting took effect: the two engines of a pair differ
    if demand is not None:
        T = net.simulation_steps
        for nid in net.origin_nodes:
            net.set_demand_matrix(nid, np.stack([demand(T, 31 * r + nid, r) for r in range(R)]))
    return net, net.engine()


def field_tensor(e, field):
    """the whole history array of `field` as the device holds it, viewed as integers (bitwise comparison: -0.0 != +0.0)"""
    cols, rs = C.c_int64(), C.c_int64()
    ptr = e._lib.pedn_device_ptr(e._h, field, C.byref(cols), C.byref(rs))
    assert ptr, e._lib.pedn_last_error(e._h).decode()
    shape = (e.history_rows(field), cols.value, rs.value)

    class Buf:
        __cuda_array_interface__ = {"data": (int(ptr), False), "shape": shape, "typestr": "<i8" if field < 7 else "<i4",
                                    "version": 2, "strides": None}

    return torch.as_tensor(Buf(), device="cuda")


def assert_same(a, b, what):
    ea, eb = a.engine(), b.engine()
    ea.synchronize(), eb.synchronize()
    (ra, fa), (rb, fb) = ea.error_flags(), eb.error_flags()
    assert ra == rb and fa.tobytes() == fb.tobytes(), what
    for f in range(N_FIELDS):
        x, y = field_tensor(ea, f), field_tensor(eb, f)
        assert x.shape == y.shape
        if not torch.equal(x, y):
            bad = torch.nonzero(x != y)
            pytest.fail(f"{what}: field {f} differs at {bad.shape[0]} entries, first [t, column, replica] = {bad[0].tolist()}")
    for node in range(ea.model["n_nodes"]):
        for r in (0, ea.n_replicas - 1):
            assert np.array_equal(ea.get_turning_fractions(node, r).view(np.int64), eb.get_turning_fractions(node, r).view(np.int64)), (what, node, r)


def pair(name, R, **kw):
    a, b = make(name, R, True, **kw)[0], make(name, R, False, **kw)[0]
    assert a.engine() is not b.engine() and a.engine().plan_info()["quiet_corridors"] and not b.engine().plan_info()["quiet_corridors"]
    return a, b


def test_quiet_corridors_follow_the_setting():
    """the default of the owner-wave plan is on; PEDN_QUIET=0 / =1 at creation decide; a model without the owner-wave plan never has them"""
    net = NetworkEnvGenerator(DATA).create_network("melbourne", verbose=False, n_replicas=64, rng_seed=5)
    if "PEDN_QUIET" not in os.environ:
        assert net.engine().plan_info()["quiet_corridors"]
    net.close()
    for q in (True, False):
        net, e = make("melbourne", 64, q)
        assert e.plan_info()["quiet_corridors"] == q
        net.close()
    keep = os.environ.get("PEDN_LINK_OWNER")
    os.environ["PEDN_LINK_OWNER"] = "0"
    try:
        net = NetworkEnvGenerator(DATA).create_network("melbourne", verbose=False, n_replicas=64, rng_seed=5)
        info = net.engine().plan_info()
    finally:
        os.environ.pop("PEDN_LINK_OWNER") if keep is None else os.environ.__setitem__("PEDN_LINK_OWNER", keep)
    assert not info["link_update_by_next_node_kernel"] and not info["quiet_corridors"], info
    net.close()


@pytest.mark.parametrize("scale", [1.0, 12.0])
def test_melbourne_1024_full_horizon(scale):
    """the headline workload (bench.py: melbourne x 1024, Poisson demand) and its congested regime, the whole horizon in one range"""
    a, b = pair("melbourne", 1024, demand=lambda T, k, r: poisson_demand(T, k, scale))
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, f"melbourne x 1024, demand x {scale}")
    a.close(), b.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_corridors_that_fill_and_empty_again(streams):
    """a short pulse of demand: corridors carry pedestrians and then empty -- their cumulative counts stay non-zero and level, and such a
    corridor must never take the quiet batch (its cumulative_outflow / cumulative_inflow are not +0.0)"""
    def pulse(T, k, r):
        d = np.zeros(T)
        d[2:12] = np.random.default_rng(k).poisson(8.0, 10)
        return d

    a, b = pair("melbourne", 256, streams=streams, demand=pulse)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, f"pulse, {streams} chain(s)")
    ci, q = a.engine().read_block(2, T - 1, T), a.engine().read_block(0, T - 1, T)   # cumulative_inflow, inflow of the last step
    assert ((ci > 0) & (q == 0)).any()      # corridors that carried pedestrians and are level again
    a.close(), b.close()


def test_single_steps_with_reads_and_setters_between():
    a, b = pair("melbourne", 256, demand=lambda T, k, r: poisson_demand(T, k))
    T = a.simulation_steps
    for n in (a, b):
        e = n.engine()
        for t in range(1, min(T, 160)):
            e.step(t)
            if t % 17 == 0:
                e.read_block(9, t - 1, t)                     # a read settles the pending link update
            if t % 29 == 0:
                e.set_width(0, 5, 1.5 + 0.01 * t)             # front gate of link 5, every replica
            if t % 41 == 0:
                nid = list(n.origin_nodes)[0]
                n.set_demand_matrix(nid, np.stack([poisson_demand(T, 999 + r, 3.0) for r in range(e.n_replicas)]))
    assert_same(a, b, "single steps with reads and setters")
    a.close(), b.close()


@pytest.mark.parametrize("lazy", [False, True])
def test_resets_mid_run_and_episode_turnover(lazy):
    a, b = pair("melbourne", 512, demand=lambda T, k, r: poisson_demand(T, k, 4.0))
    T = a.simulation_steps
    for n in (a, b):
        e = n.engine()
        e.run(1, 90)
        e.reset(lazy=lazy)                                   # mid-range: the next range starts a new episode
        e.run(1, 60)
        e.run(60, 140)
        e.reset(lazy=lazy)
        e.run(1, T)
    assert_same(a, b, f"resets (lazy={lazy})")
    a.close(), b.close()


def test_negative_flows_leave_the_group_unquiet():
    """a negative origin demand in one replica raises PEDN_F_NEG_FLOW there; from then on the quiet words of that replica's group stay
    off (a negative flow is the one way a cumulative count can fall), and the results are still those of the full batch"""
    def dip(T, k, r):
        d = poisson_demand(T, k)
        if r == 3:
            d[5:9] = -4.0
        return d

    a, b = pair("melbourne", 256, demand=dip)
    T = a.simulation_steps
    for n in (a, b):
        n.engine().run(1, T)
    assert_same(a, b, "negative demand in replica 3")
    assert a.engine().error_flags()[1][3] != 0
    a.close(), b.close()
