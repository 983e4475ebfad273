"""The engine with its default settings -- quiet corridors, zero elision and the lean quiet step all on, no PEDN_QUIET* / PEDN_ZERO_ELIDE
variable set -- against one CPU oracle per replica, under demand that makes the 64-lane votes of node_kernel<LU> come out every way
(tests/sparse_demand.py).  Every replica, every physical link, every row of all 13 history fields by bits, the error flags and the
turning fractions of every node (sparse_oracle.assert_engine_equals_oracles); test_sparse_demand_host.py checks on the CPU that the
oracle raises no flag in any of these cases and that each pattern produces the state it is there for."""
import os

import numpy as np
import pytest

import sparse_oracle as so
from golden_util import ALL_FIELDS
from pednstream_amd.network import LINK_FIELDS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_settings():
    """the point is the default engine"""
    assert not [k for k in os.environ if k.startswith("PEDN_QUIET") or k == "PEDN_ZERO_ELIDE"]


def live(net, full_history=True, chains=None):
    """the engine of `net`, with the paths under test live"""
    e = net.engine()
    info = e.plan_info()
    assert info["link_update_by_next_node_kernel"] and info["quiet_corridors"] and info["quiet_lean"], info
    assert info["zero_elide"] == full_history, info
    if chains is not None:
        assert info["chains"] == chains, info
    return e


def gated(e):
    return e.plan_info()["zero_elide_launches"]


def prepared(pattern, name, R, **kw):
    net = so.build(name, R, **kw)
    e = live(net, full_history=kw.get("history", "full") == "full")
    demand = so.demand_for(net, pattern, R, name)
    so.upload(net, demand)
    return net, e, demand, so.steps_for(pattern, so.window(net))


@pytest.mark.parametrize("pattern,name,R", so.cases())
def test_default_engine_equals_oracle(pattern, name, R):
    net, e, demand, steps = prepared(pattern, name, R)
    e.run(1, steps)
    o = so.Oracles(net, demand, R)
    o.run(1, steps)
    so.assert_engine_equals_oracles(e, o, steps, f"{pattern} on {name} x {R}")
    assert gated(e) > 0
    o.close(), net.close()


@pytest.mark.parametrize("R", [70, 192])
def test_minus_zero_is_stored(R):
    """rows that are zero in all 64 lanes, some of them -0.0: the elision votes on bits"""
    net, e, demand, steps = prepared("minus_zero", "long_corridor", R)
    e.run(1, steps)
    o = so.Oracles(net, demand, R)
    o.run(1, steps)
    so.assert_engine_equals_oracles(e, o, steps, f"minus_zero on long_corridor x {R}")
    assert gated(e) > 0
    o.close(), net.close()


@pytest.mark.parametrize("pattern,name", [("lone_lane", "fuzz_separators"), ("staggered", "long_corridor")])
def test_two_chains(pattern, name, monkeypatch):
    """256 replicas as two chains of launches: groups 0, 1 and 2, 3 step on two streams; lone_lane leaves group 3 empty"""
    monkeypatch.setenv("PEDN_STREAMS", "2")          # read when the engine is created
    monkeypatch.setenv("PEDN_STREAM_PROBE", "0")
    R = 256
    net = so.build(name, R)
    e = live(net, chains=2)
    demand = so.demand_for(net, pattern, R, name)
    so.upload(net, demand)
    steps = so.steps_for(pattern, so.window(net))
    e.run(1, steps)
    assert e.plan_info()["chains"] == 2
    o = so.Oracles(net, demand, R)
    o.run(1, steps)
    so.assert_engine_equals_oracles(e, o, steps, f"two chains, {pattern} on {name}")
    assert gated(e) > 0
    o.close(), net.close()


@pytest.mark.parametrize("pattern,name,R", [("staggered", "long_corridor", 70), ("drain_refill", "melbourne", 64), ("lone_lane", "fuzz_separators", 192)])
def test_step_by_step_with_reads_and_flushes(pattern, name, R):
    """the reference's loop; every network_loading(t) leaves its link update pending, a read or a flush settles it mid-run"""
    net, e, demand, steps = prepared(pattern, name, R)
    for t in range(1, steps):
        net.network_loading(t)
        if t % 13 == 0:
            e.read_block(LINK_FIELDS["num_pedestrians"][0], t - 1, t + 1)
        if t % 19 == 0:
            e.flush()
    o = so.Oracles(net, demand, R)
    o.run(1, steps)
    so.assert_engine_equals_oracles(e, o, steps, f"step by step, {pattern} on {name} x {R}")
    assert gated(e) > 0
    o.close(), net.close()


@pytest.mark.parametrize("name,pattern", [("fuzz_separators", "alternating"), ("long_corridor", "alternating")])
def test_per_replica_gates(name, pattern):
    """the back gate of an origin's first corridor closed in two lanes of the second group for 20 steps, then reopened"""
    R, lanes, t_close, t_open = 192, [69, 127], 12, 32
    net, e, demand, steps = prepared(pattern, name, R)
    origin = list(net.origin_nodes)[0]
    link = next(lk for (u, v), lk in net.links.items() if u == origin)
    width = float(e.model["back_gate0"][link.index])
    o = so.Oracles(net, demand, R)
    for t0, t1, w in ((1, t_close, None), (t_close, t_open, 0.0), (t_open, steps, width)):
        if w is not None:
            for r in lanes:
                e.set_width(1, link.index, w, replica=r)
            o.set_width(1, link.index, w, lanes)
        e.run(t0, t1)
        o.run(t0, t1)
    q = o.field("inflow", steps)[:, link.index, :]
    assert not q[t_close:t_open, lanes].any() and q[t_close:t_open].any() and q[t_open:, lanes].any()   # the gates mattered
    so.assert_engine_equals_oracles(e, o, steps, f"per-replica gates, {pattern} on {name}")
    o.close(), net.close()


@pytest.mark.parametrize("name,R", [("long_corridor", 70), ("fuzz_separators", 192)])
def test_lazy_and_full_reset_before_a_sparse_episode(name, R):
    """a dense episode, a lazy reset, then lone_lane: the rows still hold the dense episode's values, so no elision gate may open, and
    the bits are the oracle's after its reset.  The same after a full reset, which reopens the gates."""
    from test_gpu_quiet_corridors import poisson_demand

    net = so.build(name, R)
    e = live(net)
    T, W = net.simulation_steps, so.window(net)
    dense = {nid: np.stack([poisson_demand(T, 31 * r + k, 12.0) for r in range(R)]) for k, nid in enumerate(net.origin_nodes)}
    sparse = so.demand_for(net, "lone_lane", R, name)
    steps1, steps2 = W + 50, W + 40
    o = so.Oracles(net, dense, R)
    so.upload(net, dense)
    e.run(1, steps1)
    o.run(1, steps1)
    assert not o.flags().any()
    so.assert_engine_equals_oracles(e, o, steps1, f"dense episode on {name}")
    for lazy in (True, False):
        net.reset(lazy=lazy)
        so.upload(net, sparse)
        o.reset()
        o.set_demand(sparse)
        assert gated(e) == 0
        e.run(1, steps2)
        o.run(1, steps2)
        assert (gated(e) == 0) if lazy else (gated(e) > 0), (lazy, gated(e))
        so.assert_engine_equals_oracles(e, o, steps2, f"lone_lane on {name} after a {'lazy' if lazy else 'full'} reset")
        if lazy:                        # dirty the rows again for the full reset
            net.reset(lazy=True)
            so.upload(net, dense)
            e.run(1, steps1)
    o.close(), net.close()


@pytest.mark.parametrize("name,R", [("fuzz_separators", 70), ("melbourne", 64)])
def test_recent_history(name, R):
    """history="recent": most fields are short rings (no zero elision there); at several stops, the rows still inside every ring"""
    net, e, demand, steps = prepared("staggered", name, R, history="recent")
    o = so.Oracles(net, demand, R)
    T1 = e.T + 1
    held = {f: e.history_rows(LINK_FIELDS[f][0]) for f in ALL_FIELDS}
    assert held["inflow"] == T1 and held["sending_flow"] < T1 and held["density"] < T1
    t = 1
    for stop in (3, 17, 40, steps - 1):
        e.run(t, stop + 1)
        o.run(t, stop + 1)
        t = stop + 1
        rows = {}
        for f in ALL_FIELDS:
            newest = stop - 1 if f in ("sending_flow", "receiving_flow") else stop      # S / R of step t are entries t - 1
            rows[f] = (max(0, newest - held[f] + 2) if held[f] < T1 else 0, newest + 1)
        so.assert_engine_equals_oracles(e, o, None, f"recent history, {name} at step {stop}", rows=rows)
    assert gated(e) == 0
    o.close(), net.close()


@pytest.mark.parametrize("pattern", ["all_zero", "lone_lane"])
def test_short_links_raise_the_same_step_flag(pattern):
    """corridors with a shock-wave look-back of zero steps never turn quiet; the reference has no numbers there (sparse_oracle.SHORT_LINKS),
    engine and oracle both say so in every replica"""
    R = 70
    net, e, demand, steps = prepared(pattern, so.SHORT_LINKS, R)
    e.run(1, steps)
    o = so.Oracles(net, demand, R)
    o.run(1, steps)
    assert (o.flags() & so.F_SAME_STEP).all()
    assert np.array_equal(e.error_flags()[1] & so.F_SAME_STEP, o.flags() & so.F_SAME_STEP)
    o.close(), net.close()
