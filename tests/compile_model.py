"""Plumbing of tests/test_model_compile_host.py: the stand-alone driver of the model compiler (tests/compile_prog.cpp over
pednstream_amd/csrc/pedn_compile.hpp), the writer of its model file, and the list of models the test runs."""
import copy
import os
import subprocess

import numpy as np

from pednstream_amd.engine import ABI_VERSION, ModelDesc, _PTR_TYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEDN_E_ARG = -1


def build_prog(out_dir):
    """tests/compile_prog.cpp with the host compiler and ASan + UBSan, no HIP library; the executable's path."""
    exe = os.path.join(str(out_dir), "compile_prog")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "compile_prog.cpp")], check=True)
    return exe


def _line(name, arr, dtype):
    a = np.ascontiguousarray(arr, dtype=dtype).ravel()
    if dtype == np.int32:
        return f"{name} i {a.size} " + " ".join(map(str, a.tolist()))
    bits = a.view(np.uint64 if dtype == np.float64 else np.uint32)
    return f"{name} {'d' if dtype == np.float64 else 'f'} {a.size} " + " ".join("%x" % b for b in bits.tolist())


def write_model(m, path, dead_sets=()):
    """The fields of pedn_model_desc from the dict flatten_network returns, every array at its exact size; dead_sets: node masks for
    the live repackings."""
    import ctypes as C

    lines = []
    for name, ctype in ModelDesc._fields_:
        if name == "abi_version":
            lines.append(_line(name, [m.get("abi_version", ABI_VERSION)], np.int32))
        elif name == "node_cost":
            if m.get("node_cost") is not None:
                lines.append(_line(name, m[name], np.float32))
        elif ctype in _PTR_TYPES:
            lines.append(_line(name, m[name], _PTR_TYPES[ctype]))
        elif ctype is C.c_double:
            lines.append(_line(name, [m[name]], np.float64))
        else:
            lines.append(_line(name, [m.get(name, 0) if name in ("history_mode", "node_model") else m[name]], np.int32))
    for k, dead in enumerate(dead_sets):
        lines.append(_line(f"dead{k}", dead, np.int32))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run_prog(exe, path, n_replicas=1, **options):
    """{key: [rows of ints]}; rc and err as scalars.  Keys that end in P or are lp / corr hold hexadecimal words."""
    r = subprocess.run([exe, str(path), str(n_replicas)] + [f"{k}={v}" for k, v in options.items()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(":")
        if key == "err":
            out["err"] = rest.strip()
        elif key == "rc":
            out["rc"] = int(rest)
        else:
            base = 16 if key.endswith("P") or key in ("lp", "corr") else 10
            out.setdefault(key, []).append(np.array([int(x, base) for x in rest.split()], dtype=np.int64))
    return out


# ---------------------------------------------------------------------------------------------------------------- the models
FUZZ_SEEDS = (3, 15, 21, 40)            # fuzz_cases.random_case: with and without routes, separators, short links (21)
MUTATED_SEEDS = (4001, 4007, 4012)      # dead_link_cases.mutated_case: closed turns, zero demand rows, sparse OD weights


def star_case(arms=8):
    """a junction of `arms` corridors (PEDN_MAX_DEGREE), one origin, two destinations"""
    adj = np.zeros((arms + 1, arms + 1), dtype=int)
    adj[0, 1:] = adj[1:, 0] = 1
    default = {"length": 60.0, "width": 3.0, "free_flow_speed": 1.3, "k_critical": 2.0, "k_jam": 6.0, "gamma": 0.01, "speed_noise_std": 0.03,
               "fd_type": "yperman", "bi_factor": 1.2, "activity_probability": 0.1}
    params = {"unit_time": 10.0, "simulation_steps": 60, "assign_flows_type": "classic", "seed": 1,
              "path_finder": {"k_paths": 3, "temp": 2.0, "alpha": 1.0, "beta": 0.5, "omega": 1.0}, "default_link": default, "links": {},
              "demand": {"origin_1": {"pattern": "constant", "peak_lambda": 20.0, "base_lambda": 10.0}}}
    return adj, params, [1], [2, 3]


def model_names():
    from golden_util import DATA

    data = sorted(d for d in os.listdir(DATA) if os.path.isdir(os.path.join(DATA, d)))
    return data + [f"fuzz_{s}" for s in FUZZ_SEEDS] + [f"mutated_{s}" for s in MUTATED_SEEDS] + ["star_8"]


def model(name, history="full"):
    """the flattened model of a name of model_names()"""
    import dead_link_cases as dl
    from fuzz_cases import random_case
    from golden_util import DATA
    from pednstream_amd import Network, NetworkEnvGenerator
    from pednstream_amd.flatten import flatten_network

    if name.startswith("mutated_"):
        m = dl.mutated_case(int(name[8:]))[1]
        return dict(m, history_mode=1 if history == "recent" else 0)
    if name.startswith("fuzz_") or name == "star_8":
        seed = 1 if name == "star_8" else int(name[5:])
        adj, params, origins, dests = star_case() if name == "star_8" else random_case(seed, short_links=seed == 21)
        np.random.seed(seed)
        net = Network(adj, copy.deepcopy(params), origin_nodes=origins, destination_nodes=dests, verbose=False, n_replicas=1, rng_seed=seed, history=history)
    else:
        np.random.seed(7)
        net = NetworkEnvGenerator(DATA).create_network(name, verbose=False, n_replicas=1, history=history)
    m = flatten_network(net)
    net.close()
    return m


# ---------------------------------------------------------------------------------------------------------------- corrupted models
def wheel_case():
    """a hub of 8 corridors whose arms are joined in a ring: the smallest kind of model in which one row of fractions has eight softmax entries"""
    adj, params, _, _ = star_case(8)
    for i in range(1, 9):
        adj[i, i % 8 + 1] = adj[i % 8 + 1, i] = 1
    params["path_finder"]["k_paths"] = 4
    return adj, params, [1], [3, 4, 5, 6, 7]


def wheel_model():
    from pednstream_amd import Network
    from pednstream_amd.flatten import flatten_network

    adj, params, origins, dests = wheel_case()
    np.random.seed(1)
    net = Network(adj, copy.deepcopy(params), origin_nodes=origins, destination_nodes=dests, verbose=False, n_replicas=1, rng_seed=1)
    m = flatten_network(net)
    net.close()
    return m


def _arr(m, key):
    m[key] = np.array(m[key]).copy()
    return m[key]


def _slot_of_in(m, l):
    return int(np.flatnonzero(np.asarray(m["slot_in_link"]) == l)[0])


def _group_rows(m):
    """per softmax group: (node, row) of the products its entries feed, None for a group that feeds none"""
    ent_pair = {int(e): q for q, e in enumerate(m["pair_ent"])}
    tpp, sp, tp_ = np.asarray(m["turn_pair_ptr"]), m["node_slot_ptr"], m["node_turn_ptr"]
    rows = []
    for g in range(int(m["n_grp"])):
        n, row = int(m["grp_node"][g]), None
        for e in range(int(m["grp_ent_ptr"][g]), int(m["grp_ent_ptr"][g + 1])):
            if e in ent_pair:
                tn = int(np.searchsorted(tpp, ent_pair[e], side="right")) - 1
                row = (tn - int(tp_[n])) // int(sp[n + 1] - sp[n] - 1)
        rows.append((n, row))
    return rows


def corrupt(m, kind):
    """(a copy of the flattened model m with one fault, the message the engine refuses it with).  Every fault is chosen so that no earlier
    check of pedn_compile::validate / compile trips over it."""
    m = dict(m)
    N, L = int(m["n_nodes"]), int(m["n_links"])
    sp = np.asarray(m["node_slot_ptr"])
    virtual = int(np.flatnonzero(np.asarray(m["slot_in_link"]) >= L)[0])
    physical = int(np.flatnonzero(np.asarray(m["slot_in_link"]) < L)[0])
    if kind == "abi":
        m["abi_version"] = ABI_VERSION + 1
        return m, "pedn_model_desc.abi_version mismatch"
    if kind == "sizes":
        m["T"] = 1
        return m, "bad sizes in model description"
    if kind == "degree":
        _arr(m, "node_slot_ptr")[0] = sp[1] - 1       # node 0 keeps one slot
        return m, "node degree 1 outside 2..8"
    if kind == "one_to_one":
        _arr(m, "node_kind")[int(np.flatnonzero(np.diff(sp) > 2)[0])] = 0
        return m, "one-to-one node with degree != 2"
    if kind == "turn_ptr":
        _arr(m, "node_turn_ptr")[N] += 1
        return m, "node_turn_ptr inconsistent"
    if kind == "slot_range":
        _arr(m, "slot_in_link")[0] = -1
        return m, "slot link index out of range"
    if kind == "virtual_physical":
        _arr(m, "slot_out_link")[virtual] = 0
        return m, "virtual/physical mismatch in a slot"
    if kind == "reverse_pair":
        _arr(m, "slot_out_link")[physical] = m["slot_in_link"][physical]
        return m, "slot does not hold a reverse pair"
    if kind == "demand_row":
        _arr(m, "node_demand_row")[int(np.searchsorted(sp, virtual, side="right")) - 1] = -1
        return m, "virtual slot without demand row"
    if kind == "involution":
        # a -> b -> c with c != a, and the slot whose incoming link is b holds (b, c): every slot still holds a "reverse pair"
        a = 0
        b = int(m["link_rev"][a])
        c = next(l for l in range(L) if l not in (a, b))
        _arr(m, "link_rev")[b] = c
        _arr(m, "slot_out_link")[_slot_of_in(m, b)] = c
        return m, "link_rev is not an involution"
    if kind == "fd":
        _arr(m, "link_fd")[L - 1] = 3
        return m, "unknown fundamental diagram type"
    if kind == "group_size":
        _arr(m, "grp_ent_ptr")[int(m["n_grp"])] += 8
        return m, "softmax group too large"
    if kind == "history_mode":
        m["history_mode"] = 2
        return m, "unknown history_mode"
    if kind == "node_model":
        m["node_model"] = 2
        return m, "unknown node_model"
    if kind == "pair_ent":
        _arr(m, "pair_ent")[1] = m["pair_ent"][0]
        return m, "pair_ent is not injective"
    if kind == "grp_node":
        _arr(m, "grp_node")[0] = N
        return m, "grp_node / node_grp_ptr inconsistent"
    rows = _group_rows(m)
    if kind == "group_rows":
        # two products of different nodes change entries: each entry's group now feeds a turn of another node
        ent_grp = np.searchsorted(np.asarray(m["grp_ent_ptr"]), np.asarray(m["pair_ent"]), side="right") - 1
        qa = 0
        qb = next(q for q in range(int(m["n_pair"])) if m["grp_node"][ent_grp[q]] != m["grp_node"][ent_grp[qa]])
        pe = _arr(m, "pair_ent")
        pe[qa], pe[qb] = pe[qb], pe[qa]
        return m, "products of one softmax group lie in different rows"
    multi = [g for g in range(int(m["n_grp"])) if m["grp_ent_ptr"][g + 1] - m["grp_ent_ptr"][g] > 1 and rows[g][1] is not None
             and m["node_dyn"][rows[g][0]] and m["node_kind"][rows[g][0]] == 1]
    if kind == "ent_link":
        g = multi[0]
        n = rows[g][0]
        out = set(int(l) for l in m["slot_out_link"][sp[n]:sp[n + 1]])
        _arr(m, "ent_link")[int(m["grp_ent_ptr"][g])] = next(l for l in range(L) if l not in out)
        return m, "softmax entry is not an outgoing link of its node"
    if kind == "downstream":
        # the eight entries of one row of the hub's multi-entry groups name its eight outgoing links (a row has seven other corridors)
        hub = int(np.flatnonzero(np.diff(sp) == 8)[0])
        by_row = {}
        for g in multi:
            if rows[g][0] == hub:
                by_row.setdefault(rows[g][1], []).extend(range(int(m["grp_ent_ptr"][g]), int(m["grp_ent_ptr"][g + 1])))
        ents = next(e for e in by_row.values() if len(e) >= 8)
        _arr(m, "ent_link")[ents[:8]] = m["slot_out_link"][sp[hub]:sp[hub] + 8]
        return m, "a row refers to more than 7 downstream links"
    if kind == "no_entry":
        _arr(m, "node_dyn")[rows[multi[0]][0]] = 0      # the node's rows are not built: its products have no probability to read
        return m, "(turn, od) product without a softmax entry on a dynamic node"
    raise KeyError(kind)


VALIDATE_FAULTS = ("abi", "sizes", "degree", "one_to_one", "turn_ptr", "slot_range", "virtual_physical", "reverse_pair", "demand_row", "involution",
                   "fd", "group_size", "history_mode", "node_model")
COMPILE_FAULTS = ("pair_ent", "grp_node", "group_rows", "ent_link", "no_entry")      # on nine_intersections; "downstream" on the wheel
