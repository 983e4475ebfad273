"""The model compiler (pednstream_amd/csrc/pedn_compile.hpp) without a GPU: its stand-alone driver (tests/compile_prog.cpp), built with
AddressSanitizer + UBSan, compiles every scenario under data/, generated networks of fuzz_cases / dead_link_cases and a degree-8 star, in
both history modes and both node models and under the compiler's diagnostics knobs.  Nothing is stepped; the tables are checked for the
properties the kernels rely on, not against a frozen layout.  The refusals: one corrupted model per message."""
import numpy as np
import pytest

import compile_model as cm
import partition_model as pm

LDS_ROWS, TROW_WORDS, COOP_GROUPS, FULL = 64, 128, 8, 0x7FFFFFFF          # pedn_types.hpp
F_IN, F_OUT, F_CI, F_CO, F_S, F_R, F_GATE = range(7)
G_TT = 0
IDLE = dict(node=-1, trow=-1, act=-1, lp=-1, mirror=-1)
FIELDS = ("node", "slot", "base", "m", "kind", "dyn", "lin", "lout", "turn0", "demand_row", "act", "lp", "trow", "mirror")
BIG = ("melbourne", "delft")          # one parametrisation each


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return cm.build_prog(tmp_path_factory.mktemp("compile"))


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = cm.model(name)
        return cache[name]
    return get


def records(out, prefix):
    return [dict(zip(FIELDS, (int(x) for x in row))) for row in out[prefix + "rec"]]


def check_packing(m, out, prefix, dead=None, full=None):
    """the invariants of a packing; dead / full: a live repacking of the full packing `full` without the nodes of `dead`"""
    N, L = int(m["n_nodes"]), int(m["n_links"])
    sp = np.asarray(m["node_slot_ptr"])
    rec = records(out, prefix)
    n_blocks, tiles, n_lp, lp_max_m, n_rec = (int(x) for x in out[prefix + "info"][0])
    assert n_rec == len(rec) == (n_blocks + 1) * 8
    for R in rec[n_blocks * 8:]:          # the one trailing idle block
        assert {k: R[k] for k in IDLE} == IDLE
    where, owner, most = {}, {}, 1
    for b in range(n_blocks):
        block = rec[b * 8:b * 8 + 8]
        active = [R for R in block if R["node"] >= 0]
        assert 1 <= len(active) <= 8 and block[:len(active)] == active          # at most 8 active waves, in front
        base, w = 0, 0
        while w < len(active):          # a node's slots are consecutive waves of one block; base is the running sum of d * d
            n = active[w]["node"]
            d = int(sp[n + 1] - sp[n])
            assert n not in where and [R["node"] for R in active[w:w + d]] == [n] * d and [R["slot"] for R in active[w:w + d]] == list(range(d))
            assert all(R["base"] == base and R["m"] == d for R in active[w:w + d])
            where[n] = b * 8 + w
            base += d * d
            w += d
        most = max(most, base)
        for R in block[len(active):]:
            assert {k: R[k] for k in IDLE} == IDLE
    assert tiles == most
    live_nodes = [n for n in range(N) if dead is None or not dead[n]]
    assert sorted(where) == live_nodes          # every node of the packing once, no dead node
    for i, R in enumerate(rec):
        if R["node"] < 0:
            continue
        k = int(sp[R["node"]]) + R["slot"]
        assert (R["lin"], R["lout"]) == (int(m["slot_in_link"][k]), int(m["slot_out_link"][k]))
        if R["lin"] < L:
            assert R["lin"] not in owner
            owner[R["lin"]] = i
    if dead is None:
        assert sorted(owner) == list(range(L))          # every physical link is the incoming link of exactly one active record
    for i, R in enumerate(rec):
        if R["node"] < 0 or R["lin"] >= L:
            assert R["mirror"] == -1          # idle records and virtual pairs
        elif R["lout"] in owner:
            assert R["mirror"] == owner[R["lout"]] and rec[R["mirror"]]["mirror"] == i
        else:          # the corridor's other end is dead: the slot mirrors itself
            assert dead is not None and R["mirror"] == i
    if full is not None:          # every live node keeps its full-packing records but for base and mirror
        frec, fP = records(full, "full_"), full["full_recP"]
        fwhere = {R["node"]: i for i, R in enumerate(frec) if R["node"] >= 0 and R["slot"] == 0}
        for i, R in enumerate(rec):
            if R["node"] >= 0:
                F = frec[fwhere[R["node"]] + R["slot"]]
                assert {k: v for k, v in R.items() if k not in ("base", "mirror")} == {k: v for k, v in F.items() if k not in ("base", "mirror")}
                assert np.array_equal(out[prefix + "recP"][i], fP[fwhere[R["node"]] + R["slot"]])
    return rec, (n_lp, lp_max_m)


def check_rows(m, out, lds_limit):
    """the row and group records of turn_frac_kernel"""
    sp, tp_, tpp = np.asarray(m["node_slot_ptr"]), np.asarray(m["node_turn_ptr"]), np.asarray(m["turn_pair_ptr"])
    n_multi, n_trow, n_over = (int(x) for x in out["info"][0][:3])
    pconst, prow, slot_dyn, slot_trow = out["pair_const"][0], out["pair_row"][0], out["slot_dyn"][0], out["slot_trow"][0]
    words = out["trow_words"][0].reshape(-1, TROW_WORDS)
    groups = out["tgrp_words"][0]
    assert len(groups) == 32 * (n_multi + 8) and len(words) == max(n_trow, 1) and n_trow % 4 == 0
    groups = groups.reshape(-1, 32)
    n_pair = int(m["n_pair"])
    assert all(prow[q] >= 0 for q in range(n_pair) if not pconst[q])          # every non-constant product has somewhere to read
    named = {}
    for quad in range(n_trow // 4):
        recs = words[quad * 4:quad * 4 + 4]
        coop = recs[0][108] == 1
        if coop:          # a row with more groups than PEDN_TF_COOP_GROUPS has its workgroup to itself: four identical records
            assert all(np.array_equal(recs[0], w) for w in recs[1:])
        spans = []
        for k, w in enumerate(recs[:1] if coop else recs):
            if w[0] == -1:          # padding
                continue
            assert w[108] == coop and (w[3] > COOP_GROUPS) <= bool(w[108])
            d, ta = int(w[0]), int(w[1])
            n = int(np.searchsorted(tp_, ta, side="right")) - 1
            assert d == sp[n + 1] - sp[n] and (ta - tp_[n]) % (d - 1) == 0
            slot = int(sp[n]) + (ta - int(tp_[n])) // (d - 1)
            assert slot not in named
            named[slot] = quad * 4 + k
            assert (w[4], w[5]) == (tpp[ta], tpp[ta + d - 1])
            need = int(sum(1 for q in range(int(w[4]), int(w[5])) if not pconst[q]))
            lo, hi = int(w[109]), int(w[109]) + min(need, lds_limit)
            assert need > 0 and 0 <= lo and hi <= LDS_ROWS
            spans.append((lo, hi))
            for G in groups[int(w[2]):int(w[2]) + int(w[3])]:          # where each probability goes
                for x in G[9:16]:
                    assert x == -1 or lo <= x < hi or (LDS_ROWS <= x < LDS_ROWS + n_over), (quad, k, int(x), lo, hi, n_over)
                assert (G[9:16] >= LDS_ROWS).any() <= bool(w[107])
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans          # the LDS rows of a quad's rows are disjoint
    dyn1 = [int(k) for k in np.flatnonzero(slot_dyn == 1)]
    assert sorted(named) == dyn1          # every device-computed row has exactly one record (one quad of copies when coop) ...
    assert all(slot_trow[k] == (named[k] if k in named else -1) for k in range(len(slot_dyn)))          # ... and slot_trow points at it


def check_history(m, out):
    T1, W = int(m["T"]) + 1, int(m["window"])
    m64, m32, rows64, rows32 = (out[k][0] for k in ("m64", "m32", "rows64", "rows32"))
    for mask, rows in list(zip(m64, rows64)) + list(zip(m32, rows32)):
        assert (mask == FULL and rows == T1) or (rows == mask + 1 and rows & mask == 0 and rows < T1)
    if not int(m.get("history_mode", 0)):
        assert all(r == T1 for r in list(rows64) + list(rows32))
        return
    keeps = lambda rows, need: rows == T1 or rows >= need          # noqa: E731
    max_sw = max([int(x) for x in m["link_tau_sw"]], default=0)
    assert rows64[F_IN] == T1 and rows64[F_CI] == T1          # the sending flow looks back an unbounded number of steps into them
    assert keeps(rows64[F_CO], int(np.ceil((max_sw + 0.5) / 0.6)) + 2)          # the shock-wave look-back of a scenario with 0.6 x free-flow speed, [t'] and [t]
    assert all(keeps(rows64[f], 4) for f in (F_OUT, F_S, F_R, F_GATE))          # [t], [t - 1], [t - 2]
    assert keeps(rows32[G_TT], W + 2)          # travel_time[t - W] leaves the moving average
    assert all(keeps(rows32[g], 4) for g in range(1, 6))


def compile_and_check(prog, m, path, **options):
    N, L = int(m["n_nodes"]), int(m["n_links"])
    sp = np.asarray(m["node_slot_ptr"])
    no_virtual = np.array([all(m["slot_in_link"][k] < L for k in range(sp[n], sp[n + 1])) for n in range(N)], dtype=np.int32)
    half = (np.random.default_rng(12345).random(N) < 0.5).astype(np.int32)
    cm.write_model(m, path, [np.zeros(N, np.int32), no_virtual, half])
    out = cm.run_prog(prog, path, 1024, **options)
    assert out["rc"] == 0, out["err"]
    rec, (n_lp, lp_max_m) = check_packing(m, out, "full_")
    regular = [R for R in rec if R["node"] >= 0 and R["kind"] == 1 and R["slot"] == 0]
    if int(m.get("node_model", 0)):          # the node LP's workspace: regular nodes numbered in position order
        assert [R["lp"] for R in regular] == list(range(n_lp)) and lp_max_m == max([R["m"] for R in regular], default=0)
    assert all(R["lp"] == -1 for R in rec if R not in regular or not int(m.get("node_model", 0))) and all(R["act"] == -1 for R in rec)
    assert sorted(int(n) for n in out["pack_order"][0]) == list(range(N))
    assert int(out["info"][0][6]) == (8 if options.get("general_degree") else int(np.diff(sp).max()))
    for k, dead in enumerate((np.zeros(N, np.int32), no_virtual, half)):
        check_packing(m, out, f"live{k}_", dead=dead, full=out)
    assert [tuple(r) for r in out["live0_rec"]] == [tuple(r) for r in out["full_rec"]]
    inp = pm.proof_inputs(m)
    assert np.array_equal(out["slot_dyn"][0], inp["slot_dyn"])
    assert np.array_equal(out["pair_const"][0].astype(bool), inp["pair_const"])
    trow = {R["node"] * 8 + R["slot"]: (R["dyn"], R["trow"]) for R in rec if R["node"] >= 0}
    assert all(trow[n * 8 + k - int(sp[n])] == (out["slot_dyn"][0][k], out["slot_trow"][0][k]) for n in range(N) for k in range(sp[n], sp[n + 1]))
    check_rows(m, out, options.get("lds_limit", LDS_ROWS))
    check_history(m, out)
    assert np.array_equal(out["demand_nz"][0][:int(m["n_demand"])].astype(bool), inp["demand_nz"])
    return out


@pytest.mark.parametrize("name", cm.model_names())
def test_compiled_tables_hold_what_the_kernels_assume(prog, models, name, tmp_path):
    m = models(name)
    path = tmp_path / "model.txt"
    out = compile_and_check(prog, m, path)
    print(name, "blocks", int(out["full_info"][0][0]), "rows", int(out["info"][0][1]), "multi-entry groups", int(out["info"][0][0]))
    if name in BIG:
        return
    # the other history mode and node model, and the compiler's knobs: LDS rows per row of fractions 0 / 1 (probabilities overflow into
    # ent_p), bins by degree / by the static estimate, every quad heavy, the general node-kernel instantiation
    compile_and_check(prog, dict(m, history_mode=1), path)
    compile_and_check(prog, dict(m, node_model=1), path)
    for options in (dict(lds_limit=0), dict(lds_limit=1, pack_by_load=0), dict(pack_by_load=1, heavy_groups=0, general_degree=1)):
        knobbed = compile_and_check(prog, m, path, **options)
        if "heavy_groups" in options:
            assert int(knobbed["info"][0][3]) == max([q // 4 + 1 for q in range(0, int(knobbed["info"][0][1]), 4)
                                                      if knobbed["trow_words"][0][q * TROW_WORDS + 3] > 0] or [0])
        if options.get("lds_limit") == 0:
            assert int(knobbed["info"][0][2]) == int((knobbed["pair_row"][0][:int(m["n_pair"])] >= LDS_ROWS).sum()) or not int(m["n_pair"])


def test_a_row_with_many_groups_gets_a_workgroup_of_its_own(prog, models, tmp_path):
    """some scenario of the list has a coop row, so that check_rows' clause for it is exercised"""
    found = 0
    for name in ("delft", "45_intersections", "melbourne"):
        m = models(name)
        cm.write_model(m, tmp_path / "model.txt")
        words = cm.run_prog(prog, tmp_path / "model.txt", 1024)["trow_words"][0].reshape(-1, TROW_WORDS)
        found += int((words[:, 108] == 1).sum())
    assert found >= 4


@pytest.mark.parametrize("kind", cm.VALIDATE_FAULTS + cm.COMPILE_FAULTS + ("downstream", "row_bound"))
def test_faulty_models_are_refused_with_their_message(prog, models, kind, tmp_path):
    softmax = kind in cm.COMPILE_FAULTS or kind == "group_size"
    m = cm.wheel_model() if kind == "downstream" else models("nine_intersections" if softmax else "one_intersection_v0")
    path = tmp_path / "model.txt"
    cm.write_model(m, path)
    assert cm.run_prog(prog, path, 128)["rc"] == 0          # the intact model compiles
    if kind == "row_bound":          # (links + virtual links) x replicas rounded up to 128 reaches 2^31
        bad, msg, replicas = m, "links x replicas must stay below 2^31 (one history row)", -(-2**31 // (int(m["n_links"]) + int(m["n_vlinks"])))
        assert cm.run_prog(prog, path, replicas - 128)["rc"] == 0
    else:
        (bad, msg), replicas = cm.corrupt(m, kind), 128
    cm.write_model(bad, path)
    out = cm.run_prog(prog, path, replicas)          # (run_prog: the sanitizers stayed silent, the driver returned 0)
    assert (out["rc"], out["err"]) == (cm.PEDN_E_ARG, msg)
