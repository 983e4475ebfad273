"""The dead-link proof (pednstream_amd/csrc/pedn_partition.hpp) against the simulation itself, without a GPU.  dead_link_kernel feeds the
literal +0.0 into the step of every link the proof calls dead; here the CPU oracle -- which knows nothing of the proof -- runs random
networks with closed turns, zero demand rows and sparse OD weights (dead_link_cases.mutate) over their whole horizon, and every value
the proof fixes must be +0.0 by its bits:

  I1  a physical link outside REACH has inflow = outflow = +0.0 in every row;
  I2  at a node outside LIVE every column of its slots, incoming and outgoing, virtual ones included, has inflow, outflow and both
      cumulative counts at +0.0 in every row, and the physical ones also num_pedestrians, density, link_flow (every row) and
      sending_flow (every row a step writes: entry T - 1 keeps its initial -1.0) -- the list in dead_link_kernel's header;
  I3  the library (tests/partition_prog.cpp under ASan + UBSan) gives the same five sets as the restatement on every mutated model.

Also here: the preconditions of the literal seed list of test_gpu_dead_links_random.py, recomputed."""
import numpy as np
import pytest

import dead_link_cases as dl
import oracle_driver as od
import partition_model as pm
from sparse_oracle import bits

SEEDS = range(4000, 4300)
REPLICAS = (0, 1, 2)


def violations(m, part, o):
    """entries the proof fixes at +0.0 that the oracle has computed otherwise, in rows [0, T]"""
    dead = [n for n in range(int(m["n_nodes"])) if n not in part["live"]]
    T = int(m["T"])
    return dl.violations(m, o, dead, T + 1, unreached=[l for l in range(int(m["n_links"])) if l not in part["reach"]], sending_rows=T - 1)


@pytest.fixture(scope="module")
def campaign(tmp_path_factory):
    """every seed once: the restatement's partition, the library's, and the oracle's three replicas"""
    tmp = tmp_path_factory.mktemp("soundness")
    prog = pm.build_prog(tmp)
    res = {"ran": 0, "dropped": 0, "with_dead": 0, "with_both": 0, "runs": 0, "flagged": 0, "violations": [], "library": [], "od_zero": 0}
    for seed in SEEDS:
        case = dl.mutated_case(seed)
        if case is None:
            res["dropped"] += 1
            continue
        _, m, rec = case
        res["ran"] += 1
        inp = pm.proof_inputs(m)
        part = pm.partition(inp)
        lib = pm.run_prog(prog, inp, tmp / "model.txt")
        res["library"] += [(seed, key, sorted(lib[key] ^ part[key])[:10]) for key in part if lib[key] != part[key]]
        owner = dl.link_owner(m)
        dead_node = any(n not in part["live"] for n in owner.values())          # a node outside LIVE that has physical links
        res["with_dead"] += dead_node
        res["with_both"] += dead_node and len(part["reach"]) > 0
        res["od_zero"] += bool(((inp["slot_dyn"] == 2).any()) and rec["od_w"])
        T = int(m["T"])
        for r in REPLICAS:
            o = od.Oracle(m, seed=seed, replica=r)
            o.run(1, T)
            res["runs"] += 1
            if o.flags():
                res["flagged"] += 1        # the reference raises there: nothing behind it is defined
            else:
                assert (o.field("sending_flow")[:, T - 1:] == -1.0).all()           # the entry no step writes: -1.0
                res["violations"] += [(seed, r) + v for v in violations(m, part, o)]
            o.close()
    print({k: (v if isinstance(v, int) else len(v)) for k, v in res.items()})
    return res


def test_what_the_proof_calls_empty_is_plus_zero_in_the_oracle(campaign):
    """I1 and I2"""
    assert not campaign["violations"], (len(campaign["violations"]), campaign["violations"][:10])


def test_library_equals_the_restatement_on_the_mutated_models(campaign):
    """I3"""
    assert not campaign["library"], campaign["library"][:10]


def test_the_campaign_compares_something(campaign):
    c = campaign
    print(f"{c['ran']} ran, {c['dropped']} dropped, {c['with_dead']} with a node outside LIVE, {c['with_both']} of them with a reached link too, "
          f"{c['od_zero']} with thinned OD weights under host-tabulated rows, {c['flagged']} of {c['runs']} oracle runs flagged")
    assert c["ran"] + c["dropped"] == len(SEEDS)
    assert 3 * c["with_both"] >= c["ran"]
    assert 20 * c["flagged"] <= c["runs"]


# ---- the seed list of test_gpu_dead_links_random.py: what makes its cases mean something, recomputed here
@pytest.fixture(scope="module")
def gpu_cases():
    import test_gpu_dead_links_random as tg

    rows, kinds, narrowed_by_sep = [], set(), 0
    for i, (want, must) in enumerate(tg.EVERY):
        seed, R, mode = want[:3]
        case, m, rec = dl.mutated_case(seed)
        inp = pm.proof_inputs(m)
        part = pm.partition(inp)
        assert not (inp["slot_dyn"] == 1).any(), seed            # a row computed on the device keeps the plan off
        calls, expect = dl.call_sequence(m, R, seed, must)
        p = dl.start(case, m, rec, R, seed, mode, engines=False)
        assert p.sample == sorted({0, 63, 64, R - 1})
        p.run(1, p.T)
        assert [o.flags() for o in p.oracles] == [0] * 4, seed   # the sampled replicas raise nothing over the horizon
        p.reset()
        dl.run_calls(p, calls, expect, f"seed {seed}")           # (the oracles alone: every call is one they can follow)
        p.close()
        real = [c for c in calls if c[0] != "check"]
        assert 10 <= len(real) <= 16 and sum(c[0] == "check" for c in calls) == 2, seed
        assert all(1 <= c[3] - c[2] <= 25 and c[3] <= int(m["T"]) for c in real if c[0] == "run"), seed
        rows.append((seed, R, mode, int(m["n_nodes"]), int(m["T"]), len(part["reach"]), len(part["dead_raw"]), len(part["dead"]),
                     int((inp["slot_dyn"] == 2).any()), len(real)) + expect[-1][:2])
        if i >= len(tg.CASES):
            continue                                             # a regression seed: its row is checked, the list's conditions are not its own
        kinds |= {c[0] for c in real}
        rev, owner = m["link_rev"], dl.link_owner(m)
        narrowed_by_sep += len(part["dead"]) < len(part["dead_raw"]) and any(
            m["link_sep"][x] or m["link_tau_sw"][x] < 1 for l, n in owner.items() if n not in part["live"] for x in (l, int(rev[l])))
    return tg, rows, kinds, narrowed_by_sep


def test_gpu_seed_list_is_what_its_table_says(gpu_cases):
    tg, rows, kinds, narrowed_by_sep = gpu_cases
    cases = tg.CASES
    assert len(rows) == len(tg.EVERY)
    for (want, _), got in zip(tg.EVERY, rows):
        print(got)
        assert tuple(want) == got
    assert len(cases) >= 12 and len({c[0] for c in cases}) == len(cases)
    assert all(c[3] <= 13 and c[4] <= 160 and c[5] >= 2 and c[7] >= 2 for c in cases)
    assert sum(c[8] for c in cases) >= 4                         # host-tabulated rows
    assert narrowed_by_sep >= 4                                  # a separator or a shock-wave look-back of 0 steps at a node nobody reaches
    assert kinds >= set(dl.KINDS) | {"run", "step"}, set(dl.KINDS) - kinds


def test_a_negative_front_gate_is_a_source():
    """What the random GPU cases found: a link with a negative front gate sends a negative flow however empty it is, and a one-to-one node
    hands that on.  The mutated models with a front gate of -1.0 on two links each; the reference raises there (negative sending flow),
    the engines go on computing with and without the plan, so the oracle's values behind the flag are compared all the same."""
    ran = with_dead = 0
    bad = []
    for seed in range(4000, 4120):
        case = dl.mutated_case(seed)
        if case is None:
            continue
        m = dict(case[1])
        rng = np.random.default_rng([seed, 0xF])
        front = np.array(m["front_gate0"], dtype=np.float64)
        front[rng.choice(len(front), size=2, replace=False)] = -1.0
        m["front_gate0"] = front
        part = pm.partition(pm.proof_inputs(m))
        ran += 1
        with_dead += any(n not in part["live"] for n in dl.link_owner(m).values())
        for r in REPLICAS[:2]:
            o = od.Oracle(m, seed=seed, replica=r)
            o.run(1, int(m["T"]))
            bad += [(seed, r) + v for v in violations(m, part, o)]
            o.close()
    print(f"{ran} models with two negative front gates each, {with_dead} with a node outside LIVE")
    assert not bad, (len(bad), bad[:10])
    assert 4 * with_dead >= ran
