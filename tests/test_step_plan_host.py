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
  F  with a lazy reset in effect no node launch of t runs with valid_hi < t - 1, and afterwards valid_hi >= t"""
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
