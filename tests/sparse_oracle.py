"""Shared by test_sparse_demand_host.py (CPU) and test_gpu_sparse_activity.py (GPU): the networks and cases of the sparse-demand tests,
one CPU oracle per replica, and the bitwise comparison of an engine with those oracles.  Nothing here samples replicas or allows a
tolerance: floats are compared as integers of their width, so -0.0 != +0.0 and a NaN equals only the same NaN."""
import copy
import ctypes as C

import numpy as np

import oracle_driver as od
import sparse_demand as sd
from fuzz_cases import random_case
from golden_util import ALL_FIELDS, DATA
from pednstream_amd import Network, NetworkEnvGenerator
from pednstream_amd.engine import build_model_desc
from pednstream_amd.flatten import flatten_network
from pednstream_amd.network import LINK_FIELDS

SEED, OFFSET = 5, 3          # RNG key of replica r: (SEED, OFFSET + r), on both sides

# random_case seeds without OD pairs (static turning fractions: the owner-wave plan) that have separator links; the second one is built
# with short_links=True.  test_sparse_demand_host.py checks these properties.
FUZZ_SEPARATORS, FUZZ_SHORT_LINKS = 24, 37

# The networks whose every replica the oracle follows without an error flag.  (Order: lone_lane meets 70 replicas on fuzz_separators and
# 192 on melbourne, see cases().)
NETWORKS = ("long_corridor", "fuzz_separators", "melbourne", "nine_intersections")
# A network with short links has no oracle values to compare with: a corridor shorter than half a time step looks back zero steps, into
# the row that the step is writing, where the reference's result depends on its node order -- it raises within the first steps, and
# oracle and engine set the sticky PEDN_F_SAME_STEP in every replica from step 1 on ("Known limits"; none of the random_case
# seeds 0..2999 with short_links=True is free of it under any pattern).  What is defined there, the flag itself, is compared.
SHORT_LINKS = "fuzz_short_links"
REPLICAS = (64, 70, 192)     # one group; a second group with 6 real lanes and 58 padding lanes; three groups
F_SAME_STEP = 16


def fuzz_case(name):
    return {"fuzz_separators": (FUZZ_SEPARATORS, False), "fuzz_short_links": (FUZZ_SHORT_LINKS, True)}[name]


def build(name, R, history="full"):
    """The network `name` for R replicas (no engine yet: net.engine() creates it)"""
    if name.startswith("fuzz_"):
        seed, short = fuzz_case(name)
        adj, params, origins, dests = random_case(seed, short_links=short)
        np.random.seed(seed)
        return Network(adj, copy.deepcopy(params), origin_nodes=origins, destination_nodes=dests, verbose=False, n_replicas=R,
                       rng_seed=SEED, replica_offset=OFFSET, history=history)
    np.random.seed(7)
    return NetworkEnvGenerator(DATA).create_network(name, verbose=False, n_replicas=R, rng_seed=SEED, replica_offset=OFFSET, history=history)


def window(net):
    return int(next(iter(net.links.values())).avg_travel_time_window)


def steps_for(pattern, W):
    """W + 40 at least (never the whole horizon); staggered's last pulse starts at step 60"""
    return max(W + 40, 72) if pattern == "staggered" else W + 40


# single_ped: the pedestrians of its one busy step.  1.0 wherever one pedestrian enters a corridor; the origins of these two networks
# split their demand evenly over two exits, where floor(0.5 x 1) = 0 lets nobody in: 2.0 there puts exactly one into each exit.
SINGLE_PED = {"fuzz_separators": 2.0, "nine_intersections": 2.0}


def demand_for(net, pattern, R, name=None):
    """{node id: [R, T]} for every origin of the network (`name`: its entry of NETWORKS)"""
    T, W = int(net.simulation_steps), window(net)
    kw = {"peds": SINGLE_PED.get(name, 1.0)} if pattern == "single_ped" else {}
    return {nid: {**sd.PATTERNS, **sd.EXTRA}[pattern](T, R, key=k, W=W, **kw) for k, nid in enumerate(net.origin_nodes)}


def cases():
    """every pattern x network at one replica count each, the counts rotated across the pairs: (pattern, network, replicas)"""
    return [(p, n, REPLICAS[(i + j) % 3]) for i, p in enumerate(sd.PATTERNS) for j, n in enumerate(NETWORKS)]


def upload(net, demand):
    for nid, rows in demand.items():
        net.set_demand_matrix(nid, rows)


class Oracles:
    """One CPU oracle per replica of the batch of `net`, each with that replica's RNG key and demand ({node id: [R, T]})."""

    def __init__(self, net, demand, R, seed=SEED, offset=OFFSET):
        self.model = model = flatten_network(net)
        self.R = R
        self.index = {nid: net.nodes[nid].index for nid in net.nodes}
        desc = build_model_desc(model)
        self.all = [od.Oracle(model, seed=seed, replica=offset + r, desc=desc) for r in range(R)]
        self.set_demand(demand)

    def set_demand(self, demand):
        for nid, rows in demand.items():
            assert len(rows) == self.R
            for r, o in enumerate(self.all):
                o.set_demand(self.index[nid], rows[r])

    def set_width(self, which, link, value, replicas):
        for r in replicas:
            self.all[r].set_width(which, link, value)

    def run(self, t0, t1):
        od.run_many(self.all, t0, t1)

    def reset(self):
        for o in self.all:
            o.reset()

    def flags(self):
        return np.array([o.flags() for o in self.all], dtype=np.uint32)

    def field(self, name, t1, t0=0):
        """[t1 - t0, physical links, R]"""
        fid, L = ALL_FIELDS.index(name), int(self.model["n_links"])
        dt, ct = (np.float64, C.c_double) if fid < 7 else (np.float32, C.c_float)
        out = np.empty((self.R, L, t1 - t0), dtype=dt)
        for r, o in enumerate(self.all):          # (straight from the oracle's array: Oracle.field copies all T + 1 rows first)
            cols = o.n_all if fid < 4 else o.n_links
            whole = np.ctypeslib.as_array(C.cast(o.L.pedn_oracle_field(o.h, fid), C.POINTER(ct)), shape=(cols, o.T1))
            out[r] = whole[:L, t0:t1]
        return out.transpose(2, 1, 0)

    def tally(self):
        return np.sum([o.tally() for o in self.all], axis=0)

    def tf(self):
        """[R, n_turns]"""
        return np.stack([o.tf() for o in self.all])

    def close(self):
        for o in self.all:
            o.close()


def bits(a):
    a = np.asarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_bits(got, want, what, axes="index"):
    """got and want hold the same bits: same dtype, same shape, every element equal as an integer.  Names the first difference."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    bad = bits(got) != bits(want)
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries differ, first at {axes} = {list(first)}: "
                             f"{got[first]!r} (bits {int(bits(got)[first]):#x}) against {want[first]!r} (bits {int(bits(want)[first]):#x})")


def engine_turning_fractions(e, R=None):
    """[R, n_turns]: the fractions of every node, every replica"""
    R = e.n_replicas if R is None else R
    n_nodes = int(e.model["n_nodes"])
    return np.stack([np.concatenate([e.get_turning_fractions(n, r) for n in range(n_nodes)]) for r in range(R)])


def assert_engine_equals_oracles(e, oracles, steps, what, rows=None):
    """Every replica, every physical link, rows [0, steps) of all 13 history fields by bits; the error flags; the turning fractions of
    every node.  `rows`: {field: (first row, one past the last)} where a ring holds fewer rows (recent-history mode)."""
    assert e.n_replicas == oracles.R
    for fid, name in enumerate(ALL_FIELDS):
        assert LINK_FIELDS[name][0] == fid
        lo, hi = (0, steps) if rows is None else rows[name]
        got = e.read_block(fid, lo, hi)[:, :e.n_links, :]
        assert_same_bits(got, oracles.field(name, hi, lo), f"{what}: field {fid} ({name})", f"[t - {lo}, link, replica]")
    assert_same_bits(e.error_flags()[1], oracles.flags(), f"{what}: error flags", "[replica]")
    assert_same_bits(engine_turning_fractions(e), oracles.tf(), f"{what}: turning fractions", "[replica, turn]")
