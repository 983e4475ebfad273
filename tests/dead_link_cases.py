"""Shared by the dead-link tests (test_gpu_dead_links.py, test_gpu_dead_links_random.py, test_partition_soundness.py):

  * build / Pair: one network as two engines, the dead-link plan on (PEDN_DEAD_LINKS=1) and off, and one CPU oracle per sampled replica;
    every call goes to all of them.  Pair(engines=False) drives the oracles alone, on a machine without a GPU.
  * mutated_case: a fuzz_cases.random_case network whose flattened model gets closed turns, zero demand rows and sparse OD weights, so
    that the host proof (pedn_partition.hpp) has something to prove.
  * Proof: the test's own copy of the proof's inputs, updated call by call the way the engine documents its bookkeeping (include/pedn.h,
    pedn_hip.hip: dl_refresh), and the dead-link count the Python restatement (partition_model.py) gives for them.
  * call_sequence / run_calls: a seeded sequence of API calls and its execution."""
import copy
import os

import numpy as np

import oracle_driver as od
import partition_model as pm
import sparse_demand as sd
from fuzz_cases import random_case
from golden_util import ALL_FIELDS
from pednstream_amd import Network
from pednstream_amd.flatten import flatten_network
from sparse_oracle import assert_same_bits, bits

KEYS = ("PEDN_DEAD_LINKS", "PEDN_STREAMS", "PEDN_STREAM_PROBE", "PEDN_DEAD_STREAMS", "PEDN_DEAD_WAVES")
MIN_CHAIN_RANGE = 8          # pedn_run: shorter ranges stay on one stream (chains_for)


# ---------------------------------------------------------------------------------------------------------------- engines and oracles
def network(case, R, seed, history="full"):
    adj, params, origins, dests = case
    np.random.seed(seed)
    return Network(adj, copy.deepcopy(params), origin_nodes=list(origins), destination_nodes=list(dests), verbose=False, n_replicas=R,
                   rng_seed=seed, history=history)


def build(case, R, dead, seed, history="full", knobs=None, model=None):
    """(network, engine) of case = (adj, params, origins, dests) with the dead-link plan on or off, two chains, no stream probe.
    model: create the engine from this flattened model (a mutated one) instead of the network's own."""
    from pednstream_amd.engine import Engine

    keep = {k: os.environ.get(k) for k in KEYS}
    os.environ.update({"PEDN_DEAD_LINKS": "1" if dead else "0", "PEDN_STREAMS": "2", "PEDN_STREAM_PROBE": "0"})
    os.environ.update(knobs or {})          # PEDN_DEAD_STREAMS / PEDN_DEAD_WAVES: how the lean kernel is launched
    try:
        net = network(case, R, seed, history)
        e = net.engine() if model is None else Engine(model, n_replicas=R, seed=seed)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert e.plan_info()["chains"] == 2 and e.plan_info()["link_update_by_next_node_kernel"]
    return net, e


def closed_row(net, node, frm, closed):
    """the node's m (m - 1) fractions, uniform, but in the row of the link frm -> node the turn into node -> closed is 0.0 and the others
    share 1.0"""
    m = flatten_network(net)
    n = net.nodes[node].index
    s0, d = int(m["node_slot_ptr"][n]), int(m["node_slot_ptr"][n + 1] - m["node_slot_ptr"][n])
    tf = np.full(d * (d - 1), 1.0 / (d - 1))
    i = list(m["slot_in_link"][s0:s0 + d]).index(net.links[(frm, node)].index)
    j = list(m["slot_out_link"][s0:s0 + d]).index(net.links[(node, closed)].index)
    tf[i * (d - 1):(i + 1) * (d - 1)] = 1.0 / (d - 2)
    tf[i * (d - 1) + (j if j < i else j - 1)] = 0.0
    return n, tf


class Pair:
    """The same network with the plan on and off, and one CPU oracle per sampled replica; every call goes to all of them.
    Nodes are named by their ids in tf / demand (the hand-made tree), by their model index everywhere else."""

    def __init__(self, case, R, seed, history="full", oracle=True, knobs=None, model=None, engines=True):
        self.R = R
        if engines:
            self.nets = [build(case, R, True, seed, history, knobs, model), build(case, R, False, seed, history, None, model)]
            self.engines = [e for _, e in self.nets]
            self.on, self.off = self.engines
        else:
            self.nets, self.engines = [(network(case, R, seed, history), None)], []
        net = self.nets[0][0]
        self.net, self.T = net, int(net.simulation_steps)
        self.model = flatten_network(net) if model is None else model
        self.own = model is not None and engines      # engines created here, not by the network
        self.sample = sorted({0, 63, 64, R - 1}) if oracle else []
        self.oracles = [od.Oracle(self.model, seed=seed, replica=r) for r in self.sample]
        self.index = {nid: net.nodes[nid].index for nid in net.nodes}

    # -- the hand-made tree's calls (node ids)
    def tf(self, node, frm, closed):
        n, tf = closed_row(self.net, node, frm, closed)
        self.set_tf(n, tf)

    def demand(self, node, rows):
        self.set_demand_matrix(self.index[node], rows)

    # -- every setter, by model index
    def set_tf(self, n, tf, replica=None):
        for e in self.engines:
            e.set_turning_fractions(n, tf, replica)
        for o, r in zip(self.oracles, self.sample):
            if replica is None or replica == r:
                o.set_tf(n, tf)

    def set_demand_matrix(self, n, rows):
        for e in self.engines:
            e.set_demand_matrix(n, rows)
        for o, r in zip(self.oracles, self.sample):
            o.set_demand(n, rows[r])

    def set_demand_rows(self, n, replicas, values):
        for e in self.engines:
            e.set_demand_rows(n, replicas, values)
        for o, r in zip(self.oracles, self.sample):
            if r in list(replicas):
                o.set_demand(n, values[list(replicas).index(r)])

    def set_demand(self, n, values, replica=None):
        for e in self.engines:
            e.set_demand(n, values, replica)
        for o, r in zip(self.oracles, self.sample):
            if replica is None or replica == r:
                o.set_demand(n, values)

    def set_od_weights(self, q, values):
        for e in self.engines:
            e.set_od_weights(q, values)
        for o in self.oracles:
            v = np.ascontiguousarray(values, dtype=np.float64)
            o.L.pedn_oracle_set_od_weights(o.h, int(q), v.ctypes.data_as(od.C.POINTER(od.C.c_double)), len(v))

    def width(self, which, link, value, replica=None):
        for e in self.engines:
            e.set_width(which, link, value, replica)
        for o, r in zip(self.oracles, self.sample):
            if replica is None or replica == r:
                o.set_width(which, link, value)

    def reset(self, lazy=False):
        for e in self.engines:
            e.reset(lazy=lazy)
        for o in self.oracles:
            o.reset()

    def flush(self):
        for e in self.engines:
            e.flush()

    def drop_oracles(self):
        for o in self.oracles:
            o.close()
        self.oracles, self.sample = [], []

    def run(self, t0, t1):
        for e in self.engines:
            e.run(t0, t1)
        od.run_many(self.oracles, t0, t1) if self.oracles else None

    def step(self, t):
        for e in self.engines:
            e.step(t)
        for o in self.oracles:
            o.step(t)

    def dead(self):
        assert self.off.plan_info()["dead_links"] == 0
        return self.on.plan_info()["dead_links"]

    def split_steps(self):
        """steps that went through the lean kernel since the last reset"""
        assert self.off.plan_info()["dead_link_steps"] == 0
        return self.on.plan_info()["dead_link_steps"]

    def check(self, steps, what, oracle=True):
        fa, fb = self.on.error_flags(), self.off.error_flags()
        assert fa[0] == fb[0] and fa[1].tobytes() == fb[1].tobytes(), what
        for fid, name in enumerate(ALL_FIELDS):
            got, want = self.on.read_block(fid, 0, steps), self.off.read_block(fid, 0, steps)
            assert_same_bits(got, want, f"{what}: {name} against PEDN_DEAD_LINKS=0", "[t, column, replica]")
            for o, r in zip(self.oracles if oracle else [], self.sample):
                assert_same_bits(got[:, :self.on.n_links, r], o.field(name)[:self.on.n_links, :steps].T.astype(got.dtype), f"{what}: {name} of replica {r} against the oracle", "[t, link]")
        for o, r in zip(self.oracles if oracle else [], self.sample):
            assert int(fa[1][r]) == o.flags(), (what, r)

    def close(self):
        for net, e in self.nets:
            if self.own:
                e.close()
            net.close()
        for o in self.oracles:
            o.close()


# ---------------------------------------------------------------------------------------------------------------- mutated random networks
def base_case(seed, R=1):
    """(case, flattened model) of random_case(seed), or None where the suite drops the seed: a controller node on no OD path (KeyError,
    as in the reference) or a junction of more than 8 corridors"""
    case = random_case(seed)
    try:
        net = network(case, R, seed)
    except KeyError:
        return None
    m = flatten_network(net)
    net.close()
    return None if int(m["max_degree"]) > 8 else (case, m)


def mutate(m, seed, od_weights=True):
    """A copy of the flattened model m with
      * closed turns: at every regular, non-dynamic node of degree d >= 3, every in-slot row with probability 1/2 gets k of its d - 1
        out-turns set to exactly zero, k from 1 .. d - 2, +0.0 or -0.0 alike, and the others share 1.0;
      * zero demand rows: every row but row 0 becomes all +0.0 with probability 1/2;
      * OD weights: a third of the rows zero at every step (tabulated fractions that are exactly zero), a third zero at all but two or
        three steps (which must stay possible).
    and the record of what changed: {"tf": {node: its fractions}, "zero_rows": [...], "od_w": {od: row}}."""
    rng = np.random.default_rng([int(seed), 0xDEAD])
    m = dict(m)
    sp, tp_ = m["node_slot_ptr"], m["node_turn_ptr"]
    tf, dem, odw = np.array(m["tf_init"], dtype=np.float64), np.array(m["demand"], dtype=np.float64), np.array(m["od_w"], dtype=np.float64)
    T1 = int(m["T"]) + 1
    rec = {"tf": {}, "zero_rows": [], "od_w": {}}
    for n in range(int(m["n_nodes"])):
        d = int(sp[n + 1] - sp[n])
        if m["node_kind"][n] != 1 or m["node_dyn"][n] or d < 3:
            continue
        a = int(tp_[n])
        for i in range(d):
            if rng.random() < 0.5:
                k = int(rng.integers(1, d - 1))
                shut = rng.choice(d - 1, size=k, replace=False)
                row = np.full(d - 1, 1.0 / (d - 1 - k))
                row[shut] = np.where(rng.random(k) < 0.5, 0.0, -0.0)
                tf[a + i * (d - 1):a + (i + 1) * (d - 1)] = row
                rec["tf"][n] = None
        if n in rec["tf"]:
            rec["tf"][n] = tf[a:int(tp_[n + 1])].copy()
    for row in range(1, int(m["n_demand"])):
        if rng.random() < 0.5:
            dem[row] = 0.0
            rec["zero_rows"].append(row)
    if od_weights:
        for q in range(int(m["n_od"])):
            u = rng.random()
            if u < 2.0 / 3.0:
                row = np.zeros(T1)
                if u >= 1.0 / 3.0:
                    at = rng.choice(np.arange(1, T1), size=int(rng.integers(2, 4)), replace=False)
                    row[at] = np.where(odw[q][at] > 0.0, odw[q][at], 1.0)
                odw[q] = row
                rec["od_w"][q] = row
    m.update(tf_init=tf, demand=dem, od_w=odw)
    return m, rec


def mutated_case(seed, od_weights=True):
    """(case, mutated model, record), or None for a dropped seed"""
    base = base_case(seed)
    if base is None:
        return None
    m, rec = mutate(base[1], seed, od_weights)
    return base[0], m, rec


def demand_nodes(m):
    """{demand row: node index}"""
    return {int(r): n for n, r in enumerate(m["node_demand_row"]) if r >= 0}


def link_owner(m):
    """{physical link: the node whose slot has it as its incoming link}"""
    sp, L = m["node_slot_ptr"], int(m["n_links"])
    return {int(m["slot_in_link"][k]): n for n in range(int(m["n_nodes"])) for k in range(sp[n], sp[n + 1]) if m["slot_in_link"][k] < L}


def with_staggered_demand(m, R, replica=None):
    """The model with sparse_demand.staggered in every demand row that is not all +0.0 (key: the row) -- the row of `replica`, or for the
    proof's purposes any of them: {node index: [R, T]} and a model whose rows are those of replica 0"""
    T = int(m["T"])
    rows = {n: sd.staggered(T, R, key=row) for row, n in demand_nodes(m).items() if bits(m["demand"][row]).any()}
    dem = np.zeros_like(np.asarray(m["demand"], dtype=np.float64))
    for n, v in rows.items():
        dem[m["node_demand_row"][n], :T] = v[0]
    return rows, dict(m, demand=dem)


def start(case, m, rec, R, seed, mode, engines=True):
    """A Pair on the mutated model m of `case`.  mode "create": the engines are created from m, and derive the proof's inputs from the
    model description; "setters": they are created from the network as it is and every mutation reaches them through a setter.  Then
    sparse_demand.staggered goes into every demand row that is not zero."""
    p = Pair(case, R, seed, model=m if mode == "create" else None, engines=engines)
    if mode == "setters":
        nodes = demand_nodes(m)
        for n, tf in rec["tf"].items():
            p.set_tf(n, tf)
        for row in rec["zero_rows"]:
            p.set_demand(nodes[row], np.zeros(p.T + 1))
        for q, w in rec["od_w"].items():
            p.set_od_weights(q, w)
    for n, rows in with_staggered_demand(m, R)[0].items():
        p.set_demand_matrix(n, rows)
    return p


ALL_ROWS = ("inflow", "outflow", "cumulative_inflow", "cumulative_outflow")
PHYSICAL = ("num_pedestrians", "density", "link_flow")


def violations(m, o, nodes, rows, unreached=(), sending_rows=None):
    """What dead_link_kernel's header says the proof fixes at +0.0, looked up in an oracle: in rows [0, rows) every column of the slots of
    `nodes`, incoming and outgoing, virtual ones too, has inflow, outflow and both cumulative counts at +0.0; the physical ones also
    num_pedestrians, density, link_flow, and sending_flow in rows [0, sending_rows) (rows - 1 unless given: entry t - 1 belongs to step
    t, and what no step has written keeps its initial -1.0); the physical links `unreached` have inflow = outflow = +0.0.  Returns the entries that are not: [(invariant, field, column, first row)]."""
    L, sp = int(m["n_links"]), m["node_slot_ptr"]
    field = {f: bits(o.field(f)[:, :rows]) for f in ALL_ROWS + PHYSICAL + ("sending_flow",)}
    first = lambda a: int(np.flatnonzero(a)[0])
    out = [("I1", f, l, first(field[f][l])) for l in unreached for f in ("inflow", "outflow") if field[f][l].any()]
    for n in nodes:
        for k in range(sp[n], sp[n + 1]):
            for col in (int(m["slot_in_link"][k]), int(m["slot_out_link"][k])):
                out += [("I2", f, col, first(field[f][col])) for f in ALL_ROWS + (PHYSICAL if col < L else ()) if field[f][col].any()]
                if col < L and field["sending_flow"][col, :max(rows - 1, 0) if sending_rows is None else sending_rows].any():
                    out.append(("I2", "sending_flow", col, first(field["sending_flow"][col])))
    return out


# ---------------------------------------------------------------------------------------------------------------- the proof's inputs, tracked
class Proof:
    """The inputs of the proof as the host can know them after each call, and the count plan_info() must report.  Rules (the engine's
    documented bookkeeping, not its code): a shared row of fractions is known, a row set for one replica is not (NaN); an upload of one
    whole demand row for every replica replaces what is known of the row, any other upload can only add to it; a shared gate is known,
    a per-replica one is not; between full resets, once a step has run, the set of dead nodes only shrinks and whatever a proof has
    taken for a source or found reachable stays a source of the next one (the pedestrians are still on their way)."""

    def __init__(self, model):
        self.m = model
        self.inp = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in pm.proof_inputs(model).items()}
        self.owner = link_owner(model)
        self.grow, self.nodes = True, None
        self.src, self.reach = None, set()     # the demand rows and links that the proofs since the last full reset took for sources / reached

    def _sources(self):
        if self.grow or self.src is None:
            return self.inp["demand_nz"].copy(), set()
        return self.src | self.inp["demand_nz"], self.reach

    def partition(self):
        """the proof on the tracked inputs as they are now (nothing is kept)"""
        src, seen = self._sources()
        return pm.partition(dict(self.inp, demand_nz=src, seed_links=seen))

    def dead_nodes(self):
        """the engine's refresh: the proof, its sources kept for the next one, the set of dead nodes replaced or narrowed"""
        self.src = self._sources()[0]
        part = self.partition()
        self.reach = part["reach"]
        nodes = part["node_dead"]
        if not self.grow:
            nodes &= self.nodes
        self.nodes = nodes
        return nodes

    def dead_links(self):
        nodes = self.dead_nodes()
        if any(d == 1 for d in self.inp["slot_dyn"]):
            return 0                      # rows computed on the device: the plan is off
        return sum(n in nodes for n in self.owner.values())

    def stepped(self):
        if self.grow:
            self.dead_nodes()             # the first step after a full reset proves afresh, then the set only shrinks
        self.grow = False

    def full_reset(self):
        self.grow = True

    def set_tf(self, n, tf, replica=None):
        a, b = int(self.m["node_turn_ptr"][n]), int(self.m["node_turn_ptr"][n + 1])
        self.inp["tf_u"][a:b] = tf if replica is None and not self.m["node_dyn"][n] else np.nan

    def demand_upload(self, n, values, whole_row):
        row = int(self.m["node_demand_row"][n])
        nz = bool(bits(np.ascontiguousarray(values, dtype=np.float64)).any())
        self.inp["demand_nz"][row] = nz if whole_row else (self.inp["demand_nz"][row] or nz)

    def gate(self, which, link, value, replica=None):
        self.inp["front_u" if which == 0 else "back_u"][link] = value if replica is None else np.nan


# ---------------------------------------------------------------------------------------------------------------- call sequences
KINDS = ("open_turn", "close_turn", "tf_one_replica", "demand_matrix", "demand_rows", "demand_one", "demand_zero", "gate_dead",
         "gate_live", "gate_one_replica", "read", "flush", "reset_lazy", "reset_full")
GATES = (0.0, 0.5, -1.0, float("inf"), float("nan"))


def _setter(kind, proof, rng, R, T, t):
    """One call of `kind` that makes sense in the tracked state, or None: (kind, name of the call, arguments ...)"""
    m, inp = proof.m, proof.inp
    sp, tp_ = m["node_slot_ptr"], m["node_turn_ptr"]
    static = [n for n in range(int(m["n_nodes"])) if m["node_kind"][n] == 1 and not m["node_dyn"][n] and sp[n + 1] - sp[n] >= 3]
    zero_rows = [n for row, n in demand_nodes(m).items() if not inp["demand_nz"][row]]
    busy_rows = [n for row, n in demand_nodes(m).items() if inp["demand_nz"][row]]
    dead = sorted(l for l, n in proof.owner.items() if n in (proof.nodes or ()))
    reach = sorted(proof.partition()["reach"])
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    replica = lambda: int(pick((63, R - 1, 7)))
    pulse = lambda k: np.concatenate([np.zeros(t + 1), 3.0 + rng.poisson(6.0, 5), np.zeros(T)])[:T] * np.ones((k, 1))
    if kind in ("open_turn", "close_turn"):
        rows = []
        for n in static:
            d, a = int(sp[n + 1] - sp[n]), int(tp_[n])
            cur = inp["tf_u"][a:int(tp_[n + 1])]
            if np.isnan(cur).any():
                continue
            for i in range(d):
                row = cur[i * (d - 1):(i + 1) * (d - 1)]
                if (kind == "open_turn" and (row == 0).any()) or (kind == "close_turn" and (row != 0).sum() >= 2):
                    rows.append((n, i))
        if not rows:
            return None
        n, i = pick(rows)
        d, a = int(sp[n + 1] - sp[n]), int(tp_[n])
        tf = np.array(inp["tf_u"][a:int(tp_[n + 1])])
        row = tf[i * (d - 1):(i + 1) * (d - 1)]
        if kind == "open_turn":
            row[:] = 1.0 / (d - 1)
        else:
            row[pick(np.flatnonzero(row != 0))] = pick((0.0, -0.0))
            row[row != 0] = 1.0 / (row != 0).sum()
        return (kind, "tf", n, tf, None)
    if kind == "tf_one_replica":
        if not static:
            return None
        n = pick(static)
        d = int(sp[n + 1] - sp[n])
        tf = np.full(d * (d - 1), 1.0 / (d - 1))
        i = int(rng.integers(0, d))
        tf[i * (d - 1):(i + 1) * (d - 1)] = 1.0 / (d - 2)
        tf[i * (d - 1) + int(rng.integers(0, d - 1))] = 0.0
        return (kind, "tf", n, tf, replica())
    if kind in ("demand_matrix", "demand_rows", "demand_one"):
        if not zero_rows:
            return None
        n = pick(zero_rows)
        if kind == "demand_matrix":
            return (kind, "demand_matrix", n, int(rng.integers(100, 200)), t)
        if kind == "demand_rows":
            reps = sorted({0, 17, 63, 64, 100, R - 1})
            return (kind, "demand_rows", n, reps, pulse(len(reps)))
        return (kind, "demand", n, pulse(1)[0], replica())
    if kind == "demand_zero":
        return (kind, "demand", pick(busy_rows), np.zeros(T + 1), None) if busy_rows else None
    if kind in ("gate_dead", "gate_one_replica"):
        if not dead:
            return None
        return (kind, "gate", int(rng.integers(0, 2)), pick(dead), pick(GATES) if kind == "gate_dead" else pick(GATES[:3]),
                None if kind == "gate_dead" else replica())
    if kind == "gate_live":
        return (kind, "gate", int(rng.integers(0, 2)), pick(reach), pick(GATES), None) if reach else None
    if kind == "read":
        return (kind, "read", int(rng.integers(0, len(ALL_FIELDS))), max(0, t - 3), t) if t > 1 else None
    if kind == "flush":
        return (kind, "flush")
    return (kind, "reset", kind == "reset_lazy")


def staggered_from(T, R, key, t):
    """sparse_demand.staggered, its clock started at step t"""
    rows = np.zeros((R, T))
    rows[:, t:] = sd.staggered(T - t, R, key=key)
    return rows


def _track(proof, call, R):
    """the tracked inputs after `call`"""
    name = call[1]
    if name == "tf":
        proof.set_tf(call[2], call[3], call[4])
    elif name == "demand_matrix":
        proof.demand_upload(call[2], staggered_from(int(proof.m["T"]), R, call[3], call[4]), False)
    elif name == "demand_rows":
        proof.demand_upload(call[2], call[4], False)
    elif name == "demand":
        proof.demand_upload(call[2], call[3], call[4] is None)
    elif name == "gate":
        proof.gate(call[2], call[3], call[4], call[5])
    elif name == "reset" and not call[2]:
        proof.full_reset()
    elif name in ("run", "step"):
        proof.stepped()


def call_sequence(model, R, seed, must=()):
    """10 to 16 calls: ranges of 1 to 25 steps and single steps alternating with one call of KINDS each (those of `must` first), and
    ("check",) marks at two checkpoints.  A setter that could empty the set of dead links is drawn again, up to four times.  The first range and the last one are long enough for two chains.  Returns the calls and, per
    call, the dead-link count, the lean-kernel steps since the last reset and the dead nodes that the tracked inputs give."""
    rng = np.random.default_rng([int(seed), 0xCA11])
    proof = Proof(model)
    T = int(model["T"])
    n_calls = int(rng.integers(10, 17))
    want = list(must)
    calls, expect = [], []
    t, split = 1, 0

    def add(call):
        nonlocal t, split
        if call[1] in ("run", "step"):
            n = call[3] - call[2] if call[1] == "run" else 1
            if n >= MIN_CHAIN_RANGE and proof.dead_links() > 0:
                split += n - 1            # the first node launch of a range stays on the full bin set
            t += n
        elif call[1] == "reset":
            t, split = 1, 0
        _track(proof, call, R)
        calls.append(call)
        expect.append((proof.dead_links(), split, frozenset(proof.nodes)))

    def steps(lo, hi):
        if T - t < lo:                    # the horizon is used up: a new episode
            lazy = bool(rng.random() < 0.5)
            add(("reset_lazy" if lazy else "reset_full", "reset", lazy))
        n = min(int(rng.integers(lo, hi + 1)), T - t)
        add(("step", "step", t) if n == 1 and rng.random() < 0.5 else ("run", "run", t, t + n))

    for c in range(n_calls):
        if c == 0:
            steps(9, 25)
        elif c == n_calls - 1:
            steps(12, 25)
        elif c % 2 == 0:
            steps(1, 1) if rng.random() < 0.3 else steps(1, 25)
        else:
            call = None
            while call is None:
                kind = want.pop(0) if want else KINDS[int(rng.integers(0, len(KINDS)))]
                for _ in range(4):        # of up to four draws the first that leaves a dead link, so that most cases go on proving something
                    call = _setter(kind, proof, rng, R, T, t)
                    trial = copy.deepcopy(proof)
                    if call is None or (_track(trial, call, R), trial.dead_links())[1] > 0:
                        break
            add(call)
        if c in (n_calls // 3, 2 * n_calls // 3):
            calls.append(("check", "check", t))
            expect.append(expect[-1])
    return calls, expect


def run_calls(p, calls, expect, what):
    """The calls on a Pair.  With engines: after every call the dead-link count and the lean-kernel steps the tracked inputs give, all
    fields and flags on against off against the oracles at the checkpoints, in front of every reset and at the end.  At the same places,
    with or without engines: in every oracle, flagged or not, the columns at the tracked dead nodes hold +0.0 in every row of the episode
    (violations) -- the tracked rules themselves against the simulation.  Returns the step the last episode is at."""
    t = 1
    nodes = expect[0][2] if expect else frozenset()

    def compare(where):
        if t <= 1:
            return
        for o, r in zip(p.oracles, p.sample):
            bad = violations(p.model, o, sorted(nodes), t)
            assert not bad, (f"{what}: {where}, step {t}: the oracle of replica {r} is not +0.0 at the dead nodes {sorted(nodes)}", bad[:5])
        if p.engines:
            p.check(t, f"{what}: {where}, step {t}")

    for call, (dead, split, nodes_after) in zip(calls, expect):
        name = call[1]
        if name == "run":
            p.run(call[2], call[3])
            t = call[3]
        elif name == "step":
            p.step(call[2])
            t = call[2] + 1
        elif name == "tf":
            p.set_tf(call[2], call[3], call[4])
        elif name == "demand_matrix":
            p.set_demand_matrix(call[2], staggered_from(p.T, p.R, call[3], call[4]))
        elif name == "demand_rows":
            p.set_demand_rows(call[2], call[3], call[4])
        elif name == "demand":
            p.set_demand(call[2], call[3], call[4])
        elif name == "gate":
            if not np.isfinite(call[4]):
                p.drop_oracles()          # no defined values behind a gate that is not a number
            p.width(call[2], call[3], call[4], call[5])
        elif name == "read":
            for e in p.engines[1:]:
                assert_same_bits(p.on.read_block(call[2], call[3], call[4]), e.read_block(call[2], call[3], call[4]), f"{what}: read in mid-run, call {call}")
        elif name == "flush":
            p.flush()
        elif name == "reset":
            compare("the episode that a reset ends")
            p.reset(lazy=call[2])
            t = 1
        nodes = nodes_after
        if p.engines:
            assert p.dead() == dead, (what, "dead links after", call[:3], p.dead(), dead)
            assert p.split_steps() == split, (what, "lean-kernel steps after", call[:3], p.split_steps(), split)
        if name == "check":
            compare("checkpoint")
    compare("at the end")
    return t
