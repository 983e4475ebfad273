"""The step planner (pednstream_amd/csrc/pedn_plan.hpp) without a GPU: its stand-alone driver (tests/plan_prog.cpp), built with
AddressSanitizer + UBSan, plans seeded random scripts of library calls -- single steps in sequence, repeated and jumping, ranges as one
chain, two chains and split, RL steps, reads, setters, both resets, a zero-copy pointer, clocked sections, a change of the dead set -- for
every combination of owner-wave plan, device-computed rows, single-launch plan, recent history, node LP, agent set, quiet words and zero
elision.  Every planned launch is checked against plan_model.Shadow, a shadow of device memory per half of the replicas that is written
from what the kernels read and write:

  A  a node launch of t finds the link update of t - 1 performed exactly once since t - 1's node launch on its half (an LU launch counts as
     that one); none is left unperformed at a touch, a stand-alone fraction launch or the end of the script
  B  with device rows, a node launch of t that is not inline finds the fractions of t in tfd, computed after the last invalidation; no
     fused part is planned for row T + 1
  C  quiet words are used only if the previous node launch covering that half was a non-inline LU launch of t - 1 with the same packing
     and no touch, flush, setter, reset or change of the dead set came between
  D  a zero gate is open for row x only if x is clean on that half; never in recent-history mode or after a foreign write
  E  the chains of one step get identical plans, and the state commits once
  F  with a lazy reset in effect no node launch of t runs with valid_hi < t - 1, and afterwards valid_hi >= t

The plan chooser of the same header (choose: which plan an engine steps under at all) runs through the same driver over the full grid of
plan_model.grid_spec: the implications the engine relies on, the rules as documented, the plans of the shipped scenarios, and that
plan_model.all_caps -- the combinations the planner is tested under -- holds every combination the chooser can produce."""
import numpy as np
import pytest

import plan_model as pm

SEEDS = 16          # scripts per combination: 144 combinations, about 2500 scripts of at most 40 events


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return pm.build_prog(tmp_path_factory.mktemp("plan"))


def test_every_planned_launch_finds_what_its_kernel_needs(prog, tmp_path):
    # (the few combinations that can take the split plan get eight times the scripts)
    scripts = [(caps, pm.random_script(caps, owner, 1000 * i + seed)) for i, (caps, owner) in enumerate(pm.all_caps())
               for seed in range(SEEDS * (8 if owner and pm.split_possible(caps) else 1))]
    assert all(len(events) <= 40 and caps["T1"] - 1 <= 24 for caps, events in scripts)
    results = pm.run_prog(prog, scripts, tmp_path / "scripts.txt")
    seen = dict(steps=0, lu=0, inl=0, use=0, live_use=0, zg64=0, zg32=0, flush=0, tf=0, fused=0, split=0, clear=0, refused=0, clocked=0)
    for (caps, events), result in zip(scripts, results):
        try:
            seen["steps"] += pm.check_script(caps, events, result)
        except AssertionError as e:
            raise AssertionError(f"{e}\ncaps {caps}\n" + "\n".join(f"{ev}  ->  {r[0]}" for ev, r in zip(events, result))) from None
        for launches, _ in result:
            for kind, a in launches:
                seen["flush"] += kind == "flush"
                seen["tf"] += kind == "tf"
                seen["clear"] += kind == "clear"
                seen["refused"] += kind == "refused"
                seen["split"] += kind == "lean"
                if kind == "node":
                    for k in ("lu", "inl", "use", "zg64", "zg32"):
                        seen[k] += a[k]
                if kind == "live":
                    seen["live_use"] += a["use"]
                if kind == "second":
                    seen["fused"] += a["fused"]
                    seen["clocked"] += a["obs"] and a["link"] and not a["ctrl"]
    print(len(scripts), "scripts", seen)
    assert len(scripts) >= 2000 and all(v > 50 for v in seen.values()), seen          # every path of the planner was taken, often


def test_a_session_of_library_calls_is_planned_as_documented(prog, tmp_path):
    """the fixed session of tests/test_gpu_step_plan.py under the plans a machine can report: what the planner counts for it"""
    calls = [("reset",), ("run", 1, 10), ("read",), ("step", 10), ("step", 11), ("step", 12), ("run", 13, 21)]
    caps = dict(node_lp=0, inline_tf=0, inline_help=0, quiet=1, quiet_lean=1, fuse_tp=1, fuse_obs=1, rl_ready=0, zero_elide=1, hist=0, pr=0, trow=0, links=1,
                live=1, T1=61)
    want = {(1, 0): (0, 0), (2, 0): (0, 0), (2, 7): (0, 15)}          # (chains, dead links): (nothing to compare yet, split steps)
    for (chains, dead), (_, split_steps) in want.items():
        events = pm.session_events(chains, True, dead, calls) + ["flush"]          # (a read behind the session, for rule A)
        result = pm.run_prog(prog, [(caps, events)], tmp_path / "session.txt")[0]
        pm.check_script(caps, events, result)
        state = result[-2][1]
        assert state["last_t"] == 20 and state["step_epoch"] == 21 and state["split_steps"] == split_steps
        assert state["zgated"] > 0 and state["link_pending"] == 20


# ---------------------------------------------------------------------------------------------------------------- the plan chooser
@pytest.fixture(scope="module")
def grid(prog, tmp_path_factory):
    g = pm.run_choose(prog, pm.grid_spec(), tmp_path_factory.mktemp("choose") / "grid.txt")
    keep = ~((g["inline_tf_ok"] == 1) & (g["n_trow"] == 0))          # (the compiler gives no such tables: plan_model.GRID_INPUTS)
    return {k: v[keep] for k, v in g.items()}


def implies(a, b):
    return bool(np.all(~np.asarray(a, bool) | np.asarray(b, bool)))


def knob(g, name, default):
    k = g["k_" + name]
    return np.where(k >= 0, k, default)


def test_the_grid_reaches_every_edge_and_every_knob_value(grid):
    g = grid
    assert len(g["RS"]) >= 300000
    product = g["RS"] // 64 * g["n_blocks"]
    assert set(np.unique(g["RS"])) == {128, 576, 640, 704} and 352 in product and product.max() > 352 and product.min() >= 352
    assert {64 << 10, (64 << 10) + 512, 160 << 10, (160 << 10) + 512} <= set(np.unique(g["node_lds_tf"]))          # at and one tile above both limits
    for k, values in pm.KNOBS.items():
        assert set(np.unique(g["k_" + k])) == set(values), k
    for k in ("lds_tf", "lds_h", "inline_tf_ok", "node_lp", "hist", "links", "inline_tf", "inline_help", "dead_capable", "quiet", "link_owner"):
        assert set(np.unique(g[k])) == {0, 1}, k


def test_the_chooser_keeps_what_the_engine_relies_on(grid):
    g = grid
    assert implies(g["inline_help"], g["inline_tf"]) and implies(g["inline_tf"], g["link_owner"])
    assert implies(g["inline_tf"], (g["node_lp"] == 0) & (g["inline_tf_ok"] == 1) & (g["n_trow"] > 0))
    for conjunct in (g["dead_links"], g["quiet"], g["link_owner"], g["inline_tf"] == 0, g["hist"] == 0, g["node_lp"] == 0, g["n_trow"] == 0, g["L"] > 0,
                     g["quiet_words_live"] // 2 < 2**31, g["quiet_words_live"] > 0):
        assert implies(g["dead_capable"], conjunct)
    assert np.all((g["dead_waves"] >= 3) & (g["dead_waves"] <= 8)) and np.all(np.isin(g["dead_streams"], (1, 2)))
    assert np.all(np.isin(g["chains"], (1, 2))) and np.all(np.isin(g["rl_chains"], (0, 1, 2)))
    assert np.all(g["tf_lds_off"] * 8 == g["node_lds"])
    # LDS: 8 (node LP: 16) rows of 64 doubles + the tiles; <.., TF>: + the eight slot waves' own rows
    assert np.all(g["node_lds"] == (np.where(g["node_lp"] == 1, 16, 8) + g["tiles"]) * 512)
    assert np.all(g["node_lds_tf"] == g["node_lds"] + 8 * pm.TF_WAVE_LDS * 8)
    # the plan a step is planned under is the chosen one, and the report is derived from it alone
    for k in ("node_lp", "hist", "inline_tf", "inline_help", "quiet", "quiet_lean", "fuse_tp", "fuse_obs", "zero_elide"):
        assert np.array_equal(g["c_" + k], g[k]), k
    owner_wave = g["link_owner"] & (g["node_lp"] == 0) & g["links"]
    assert np.array_equal(g["r_owner_wave"], owner_wave) and np.array_equal(g["r_quiet"], g["quiet"] & owner_wave)
    assert np.array_equal(g["r_zero_elide"], g["zero_elide"] & (g["hist"] == 0)) and np.array_equal(g["r_quiet_lean"], g["quiet_lean"] & g["quiet"] & owner_wave)
    assert np.array_equal(g["r_dead_links"], g["dead_capable"] & g["links"])


def test_the_chooser_follows_its_documented_rules(grid):
    g = grid
    large = g["node_lds_tf"] > (64 << 10)
    candidate = (g["inline_tf_ok"] == 1) & (g["node_lp"] == 0) & (g["node_lds_tf"] <= (160 << 10))
    assert np.array_equal(g["inline_candidate"], candidate)
    possible = candidate & (~large | (g["lds_tf"] == 1))
    by_grid = possible & (g["RS"] // 64 * g["n_blocks"] <= 352)
    k = g["k_inline_tf"]
    inline_tf = np.where(k < 0, by_grid, (k != 0) & possible)
    assert np.array_equal(g["inline_tf"], inline_tf)
    assert np.array_equal(g["inline_help"], np.where(k < 0, by_grid, (k == 2) & possible) & (~large | (g["lds_h"] == 1)))
    assert np.array_equal(g["link_owner"], inline_tf | knob(g, "link_owner", (g["n_trow"] == 0) & (g["node_lp"] == 0)))
    assert np.array_equal(g["quiet"], knob(g, "quiet", g["link_owner"] & (g["node_lp"] == 0)))
    assert np.array_equal(g["chains"], knob(g, "streams", np.where(g["RS"] >= 640, 2, 1)))
    for name, default in (("fuse_tp", 1), ("fuse_obs", 1), ("quiet_lean", 1), ("zero_elide", 1), ("rl_chains", 0), ("dead_links", 1), ("dead_waves", 5),
                          ("dead_streams", 1), ("stream_probe", 1)):
        assert np.array_equal(g[name], knob(g, name, default)), name
    groups = g["RS"] // 64
    assert np.array_equal(g["quiet_words"], g["quiet"] * 2 * g["n_rec"] * groups * 2)
    live_words = 2 * (g["N"] + 1) * 8 * groups * 2
    capable = (g["dead_links"] & g["quiet"] & g["link_owner"] & (g["inline_tf"] == 0) & (g["hist"] == 0) & (g["node_lp"] == 0) & (g["n_trow"] == 0) & (g["L"] > 0)
               & (live_words // 2 < 2**31))
    assert np.array_equal(g["dead_capable"], capable) and np.array_equal(g["quiet_words_live"], capable * live_words)


def test_a_device_fact_turned_off_changes_only_what_hangs_on_it(prog, tmp_path):
    """choose is called again where a request for LDS was refused: nothing but inline_help may move with lds_h, and nothing at all where
    no request would have been made (node_lds_tf within the default 64 KB, or no helper waves chosen)"""
    spec = [(k, v) for k, v in pm.grid_spec() if k not in ("lds_h", "~links")]          # (same points, same drawn knobs in both runs)
    on, off = (pm.run_choose(prog, spec + [("lds_h", h), ("links", 1)], tmp_path / f"h{h}.txt") for h in (1, 0))
    moved = [k for k in on if k not in ("lds_h", "inline_help", "c_inline_help") and not np.array_equal(on[k], off[k])]
    assert not moved, moved
    asked = (on["inline_help"] == 1) & (on["node_lds_tf"] > (64 << 10))
    assert np.array_equal(off["inline_help"], on["inline_help"] & ~asked) and asked.any() and (on["inline_help"] & ~asked).any()


def test_the_overflow_of_the_quiet_words_is_visible_in_the_plan(prog, tmp_path):
    """2^30 / (RS / 64) slot records are the first that pedn_create refuses ("too many quiet words"); so many nodes that the LIVE packing's
    words would not index in 31 bits only turn the dead-link plan off"""
    base = dict(RS=128, L=5, n_rec=(1 << 29) - 1, N=10, tf_wave_lds=pm.TF_WAVE_LDS)
    fits = pm.choose_one(prog, base, {}, tmp_path / "a.txt")
    over = pm.choose_one(prog, dict(base, n_rec=1 << 29), {}, tmp_path / "b.txt")
    assert fits["quiet"] and fits["quiet_words"] // 2 == 2**31 - 4 and over["quiet_words"] // 2 == 2**31
    cap = 2**31 // (8 * 2 * 2)          # live records (N + 1) * 8, two groups, two words
    few, many = (pm.choose_one(prog, dict(base, n_rec=24, N=n), {}, tmp_path / "c.txt") for n in (cap - 2, cap - 1))
    assert few["dead_capable"] and few["quiet_words_live"] // 2 == 2**31 - 32 and not many["dead_capable"] and many["quiet_words_live"] == 0


def test_every_caps_combination_the_chooser_produces_is_one_the_planner_is_tested_under(grid):
    g = grid
    have = {(owner, caps["trow"], caps["inline_tf"], caps["hist"], caps["node_lp"], caps["quiet"], caps["zero_elide"]) for caps, owner in pm.all_caps()}
    made = np.unique(np.stack([g["link_owner"], (g["n_trow"] > 0).astype(np.int64), g["inline_tf"], g["hist"], g["node_lp"], g["quiet"], g["zero_elide"]], 1), axis=0)
    missing = [tuple(int(x) for x in row) for row in made if tuple(int(x) for x in row) not in have]
    assert not missing, missing
    assert len(made) == 72          # all seven crossed, but for the single-launch plan without device rows, owner waves or the classic node model
    # (the entries all_caps cycles instead of crossing: each value the chooser gives occurs under it)
    for k in ("inline_help", "quiet_lean", "fuse_tp", "fuse_obs"):
        assert set(np.unique(g[k])) <= {caps[k] for caps, _ in pm.all_caps()}, k


# what pedn_create chooses for the shipped scenarios without a knob; (RS / 64) * n_blocks is printed by the test
SHIPPED = {
    # no row of fractions computed on the device: owner-wave plan with quiet words, two chains from 640 replicas, the dead-link plan possible
    ("melbourne", 1024): dict(chains=2, link_owner=1, inline_tf=0, inline_help=0, quiet=1, dead_capable=1),
    # device rows, 16 x 112 workgroups: two launches per step, no owner waves
    ("delft", 1024): dict(chains=2, link_owner=0, inline_tf=0, inline_help=0, quiet=0, dead_capable=0),
    # device rows that fit one wave each, 4 x 4 workgroups: the single-launch plan with helper waves on one chain
    ("nine_intersections", 256): dict(chains=1, link_owner=1, inline_tf=1, inline_help=1, quiet=1, dead_capable=0),
    # 23 blocks: 16 x 23 = 368 and 32 x 23 = 736 workgroups, both above 352 -- two launches per step
    ("45_intersections", 1024): dict(chains=2, link_owner=0, inline_tf=0, inline_help=0, quiet=0, dead_capable=0),
    ("45_intersections", 2048): dict(chains=2, link_owner=0, inline_tf=0, inline_help=0, quiet=0, dead_capable=0),
}
EVERYWHERE = dict(fuse_tp=1, fuse_obs=1, quiet_lean=1, zero_elide=1, rl_chains=0, dead_links=1, dead_waves=5, dead_streams=1, stream_probe=1, node_lp=0, hist=0)


def test_the_shipped_scenarios_get_their_documented_plans(prog, tmp_path):
    import compile_model as cm

    compiler = cm.build_prog(tmp_path)
    models = {}
    for (name, replicas), want in SHIPPED.items():
        m = models.setdefault(name, cm.model(name))
        cm.write_model(m, tmp_path / "model.txt")
        inputs, _ = pm.compiled_inputs(cm.run_prog(compiler, tmp_path / "model.txt", replicas), m, replicas)
        plan = pm.choose_one(prog, inputs, {}, tmp_path / "one.txt")
        print(name, replicas, "workgroups", inputs["RS"] // 64 * inputs["n_blocks"], "inline_tf_ok", inputs["inline_tf_ok"], "node_lds_tf", plan["node_lds_tf"])
        assert {k: plan[k] for k in {**want, **EVERYWHERE}} == {**want, **EVERYWHERE}, (name, replicas)
        assert plan["r_owner_wave"] == want["link_owner"] and plan["r_quiet"] == want["quiet"] and plan["r_dead_links"] == want["dead_capable"]
