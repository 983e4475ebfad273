"""The dead-link proof (pednstream_amd/csrc/pedn_partition.hpp) restated in Python, and the plumbing to ask the C++ function itself
through its stand-alone driver tests/partition_prog.cpp.

proof_inputs(m) derives from a flattened model what the engine hands the proof (pedn_hip.hip: dl_refresh): which demand rows hold anything
but +0.0, the shared fractions, where each slot's row of fractions comes from (pedn_compile.hpp: a row of a dynamic node whose (turn, od)
products are all the constant 1 is tabulated on the host, dyn = 2) and which of those tabulated fractions can be non-zero
(tabulate_pair_pod + finish_tabulated_rows).  partition(inp) is the propagation itself, written from the rules of the issue, not from
the C++."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_prog(out_dir):
    """tests/partition_prog.cpp with the host compiler and ASan + UBSan; the executable's path.  The compiler is the one the oracle's
    build uses ($CXX, else g++); a machine without it fails here, it does not skip."""
    exe = os.path.join(str(out_dir), "partition_prog")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "partition_prog.cpp")], check=True)
    return exe


def _bits_not_plus_zero(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) != 0


def _is_zero(x):
    return x == 0.0          # +-0.0; NaN compares unequal


def proof_inputs(m):
    N, L, T1 = int(m["n_nodes"]), int(m["n_links"]), int(m["T"]) + 1
    sp, tp_ = m["node_slot_ptr"], m["node_turn_ptr"]
    nt = int(m["n_turns"])
    inp = {"n_nodes": N, "n_links": L, "node_lp": int(m["node_model"]) == 1, "per_replica": False,
           "node_slot_ptr": sp, "node_turn_ptr": tp_, "node_kind": m["node_kind"], "node_demand_row": m["node_demand_row"],
           "slot_in": m["slot_in_link"], "slot_out": m["slot_out_link"], "link_rev": m["link_rev"],
           "demand_nz": np.array([_bits_not_plus_zero(row).any() for row in m["demand"]], dtype=bool),
           "link_sep": m["link_sep"], "link_tau_sw": m["link_tau_sw"], "front_u": np.array(m["front_gate0"], dtype=np.float64),
           "back_u": np.array(m["back_gate0"], dtype=np.float64), "link_rl": np.zeros(L, dtype=bool)}
    tf_u = np.array(m["tf_init"], dtype=np.float64)
    # (turn, od) products whose P(down | up, od) is the constant 1: the only entry of its softmax group (pedn_compile.hpp)
    n_pair = int(m["n_pair"])
    xmax = abs(m["pf_temp"]) * (abs(m["pf_alpha"]) + abs(m["pf_beta"]) * 16.0 + abs(m["pf_omega"]) + abs(m["pf_eps"]))
    gptr = np.asarray(m["grp_ent_ptr"])
    pconst = np.zeros(max(n_pair, 1), dtype=bool)
    for q in range(n_pair):
        g = int(np.searchsorted(gptr, m["pair_ent"][q], side="right")) - 1
        pconst[q] = (gptr[g + 1] - gptr[g] == 1) and xmax < 600.0
    tpp = np.asarray(m["turn_pair_ptr"])
    # P(od | up)[t] per (up, od) entry, then the raw fraction of every turn whose products are all constant
    upod = np.zeros((len(m["upod_od"]), T1))
    for u in range(int(m["n_up"])):
        a, b = int(m["up_od_ptr"][u]), int(m["up_od_ptr"][u + 1])
        w = np.asarray(m["od_w"], dtype=np.float64)[np.asarray(m["upod_od"][a:b])]          # [b - a][T1]
        tot = w.sum(axis=0)
        upod[a:b] = np.where(tot > 0.0, w / np.where(tot > 0.0, tot, 1.0), 1.0 / max(b - a, 1))
    slot_dyn = np.zeros(len(m["slot_in_link"]), dtype=np.int32)
    tab_nz = np.zeros(max(nt, 1), dtype=bool)
    for n in range(N):
        if m["node_kind"][n] != 1 or not m["node_dyn"][n]:
            continue
        d = int(sp[n + 1] - sp[n])
        tf_u[tp_[n]:tp_[n + 1]] = np.nan       # a dynamic node's rows are per replica
        for i in range(d):
            ta = int(tp_[n]) + i * (d - 1)
            need = int((~pconst[tpp[ta]:tpp[ta + d - 1]]).sum()) if n_pair else 0
            slot_dyn[sp[n] + i] = 1 if need else 2
            if need:
                continue
            raw = np.zeros((d - 1, T1))
            for jj in range(d - 1):
                for q in range(int(tpp[ta + jj]), int(tpp[ta + jj + 1])):
                    raw[jj] += upod[m["pair_upod"][q]]
            rowsum = raw.sum(axis=0)
            fix = np.abs(rowsum - 1) > 1e-3
            fin = np.where(fix, np.where(rowsum > 1e-6, raw / np.where(rowsum > 1e-6, rowsum, 1.0), 1.0 / (d - 1)), raw)
            tab_nz[ta:ta + d - 1] = (~_is_zero(fin)).any(axis=1)
    inp.update(tf_u=tf_u, slot_dyn=slot_dyn, tab_nz=tab_nz, pair_const=pconst)   # (pair_const: for tests/test_model_compile_host.py)
    return inp


def partition(inp):
    """REACH (links), LIVE (nodes), DEAD before eligibility (links), the nodes and links the lean kernel steps."""
    N, L = inp["n_nodes"], inp["n_links"]
    sp, tp_ = inp["node_slot_ptr"], inp["node_turn_ptr"]
    owner = {}
    for n in range(N):
        for k in range(sp[n], sp[n + 1]):
            if inp["slot_in"][k] < L:
                owner[int(inp["slot_in"][k])] = (n, k - sp[n])

    def possible(n, i, j):
        d = sp[n + 1] - sp[n]
        if inp["node_kind"][n] == 0 or inp["node_lp"]:
            return True
        dyn = inp["slot_dyn"][sp[n] + i]
        if dyn == 1:
            return True
        tn = tp_[n] + i * (d - 1) + (j if j < i else j - 1)
        if dyn == 2:
            return bool(inp["tab_nz"][tn])
        return not _is_zero(inp["tf_u"][tn])

    reach, live, todo = set(), set(), []
    for n in range(N):
        row = inp["node_demand_row"][n]
        if row >= 0 and inp["demand_nz"][row]:
            live.add(n)
            todo += [(n, k - sp[n]) for k in range(sp[n], sp[n + 1]) if inp["slot_in"][k] >= L]
    # two more kinds of source: a front gate that is, or in some replica may be, negative (the link sends a negative flow however empty
    # it is), and what an earlier proof has reached since the histories were last cleared (its pedestrians are still walking)
    for l in range(L):
        if l not in reach and (l in inp.get("seed_links", ()) or not inp["front_u"][l] >= 0):
            reach.add(l)
            todo.append(owner[l])
    while todo:
        n, i = todo.pop()
        for j in range(sp[n + 1] - sp[n]):
            lo = int(inp["slot_out"][sp[n] + j])
            if j != i and lo < L and lo not in reach and possible(n, i, j):
                reach.add(lo)
                todo.append(owner[lo])
    for l in reach:
        live.add(owner[l][0])
        live.add(owner[int(inp["link_rev"][l])][0])

    def eligible(l):
        if inp["per_replica"]:
            return False
        for x in (l, int(inp["link_rev"][l])):
            f, b = inp["front_u"][x], inp["back_u"][x]
            if inp["link_sep"][x] or inp["link_tau_sw"][x] < 1 or inp["link_rl"][x]:
                return False
            if not (np.isfinite(f) and f >= 0 and np.isfinite(b) and b >= 0):
                return False
        return True

    node_dead = set()
    for n in range(N):
        phys = [int(inp["slot_in"][k]) for k in range(sp[n], sp[n + 1]) if inp["slot_in"][k] < L]
        if n not in live and phys and all(eligible(l) for l in phys):
            node_dead.add(n)
    dead_raw = {l for l, (n, _) in owner.items() if n not in live}
    dead = {l for l, (n, _) in owner.items() if n in node_dead}
    return {"reach": reach, "live": live, "dead_raw": dead_raw, "node_dead": node_dead, "dead": dead}


def _hex(a):
    return " ".join("%x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0] for x in a)


def _ints(a):
    return " ".join(str(int(x)) for x in a)


def run_prog(exe, inp, path):
    """The same question put to pedn_part::partition through the stand-alone driver."""
    lines = [_ints([inp["n_nodes"], inp["n_links"], len(inp["slot_in"]), len(inp["tf_u"]), len(inp["demand_nz"]), inp["node_lp"], inp["per_replica"]])]
    for key in ("node_slot_ptr", "node_turn_ptr", "node_kind", "node_demand_row", "slot_in", "slot_out", "link_rev", "slot_dyn", "demand_nz"):
        lines.append(_ints(inp[key]))
    lines.append(_hex(inp["tf_u"]))
    lines.append(_ints(inp["tab_nz"][:len(inp["tf_u"])]))
    lines += [_ints(inp["link_sep"]), _ints(inp["link_tau_sw"]), _hex(inp["front_u"]), _hex(inp["back_u"]), _ints(inp["link_rl"])]
    lines.append(_ints([l in inp.get("seed_links", ()) for l in range(inp["n_links"])]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, "model", str(path)], check=True, capture_output=True, text=True).stdout
    res = {}
    for line in out.splitlines():
        key, _, rest = line.partition(":")
        res[key] = {int(x) for x in rest.split()}
    return res
