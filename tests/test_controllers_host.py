"""Rule-based controllers on the host (pednstream_amd.agents / .evaluation) against fixtures recorded with the reference's own
rl/agents/rule_based.py (tools/gen_controller_goldens.py), their refusals, the C-ABI additions and the device kernels' resources."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest

from golden_util import GOLDEN, ROOT
from pednstream_amd.agents import RuleBasedGaterAgent, RuleBasedSeparatorAgent
from pednstream_amd.evaluation import evaluate_agents, summarize_runs

CTRL_CASES = ["ctrl_nine_gate3", "ctrl_one_gate3", "ctrl_small_gate08", "ctrl_nine_gate3_g2n", "ctrl_corridor_sep",
              "ctrl_corridor_sep_smooth", "ctrl_corridor_sep_smooth_2ep",
              # a gater with 8 links (threshold 3 and 0.0) and moving-average windows other than 5 (tests/test_wide_agents_host.py)
              "ctrl_hub8_gate", "ctrl_hub8_gate0", "ctrl_corridor_sep_w1", "ctrl_corridor_sep_w8", "ctrl_corridor_sep_w13",
              "ctrl_corridor_sep_w32"]


def load(case):
    z = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["info_json"]))


def host_agents(info, links_of=None):
    """The fixture's agents as pednstream_amd.agents objects; links_of(agent_id) -> link objects (default: stand-ins with the
    recorded ids and widths)."""
    spec = {a["id"]: a for a in info["rl"]["agents"]}
    out = {}
    for aid, c in info["controllers"].items():
        if c["kind"] == "gate":
            links = links_of(aid) if links_of else [types.SimpleNamespace(link_id=l, width=w) for l, w in zip(spec[aid]["links"], c["widths"])]
            out[aid] = RuleBasedGaterAgent(links, info["rl"]["obs_mode"], threshold_density=c["threshold"])
        else:
            out[aid] = RuleBasedSeparatorAgent(c["width"], use_smoothing=c["use_smoothing"], buffer_size=c["buffer_size"])
    return out


def slices(info):
    """(action slice, observation slice) per agent id in the row layout of VecPedNetEnv (4 features per link in option2)."""
    res, a0, o0 = {}, 0, 0
    for a in info["rl"]["agents"]:
        na = 1 if a["type"] == "sep" else len(a["links"])
        res[a["id"]] = (slice(a0, a0 + na), slice(o0, o0 + 4 * na))
        a0, o0 = a0 + na, o0 + 4 * na
    return res


@pytest.mark.parametrize("case", CTRL_CASES)
def test_take_action_reproduces_every_recorded_action(case):
    """Every action of the reference's agent, from the observation it was given, bit for bit -- the moving-average buffer carried
    across the reset in the two-episode fixture."""
    z, info = load(case)
    acts, obs, reset_obs, episode = (z["state_ctrl_" + k] for k in ("actions", "obs", "reset_obs", "episode"))
    agents = host_agents(info)
    sl = slices(info)
    for k in range(len(acts)):
        prev = reset_obs[episode[k]] if k == 0 or episode[k] != episode[k - 1] else obs[k - 1]
        for aid, (sa, so) in sl.items():
            if aid not in agents:
                assert np.isnan(acts[k, sa]).all()
                continue
            a = agents[aid].take_action(prev[so], deterministic=True)
            assert a.dtype == np.float32
            assert a.tobytes() == acts[k, sa].tobytes(), (case, k, aid, a, acts[k, sa])


def test_fixtures_cover_both_branches_of_each_rule():
    """The gater fixtures take the per-link rule and the "open" branch; the separator ones return the full width and other values."""
    for case in ("ctrl_nine_gate3", "ctrl_one_gate3", "ctrl_small_gate08"):
        z, info = load(case)
        sl = slices(info)
        acts, obs = z["state_ctrl_actions"], z["state_ctrl_obs"]
        open_, rule = 0, 0
        for aid, c in info["controllers"].items():
            sa, so = sl[aid]
            dens = obs[:-1, so][:, 2::4]
            m = np.array([np.mean(list(d)) for d in dens])
            open_ += int((m <= 2).sum())
            rule += int((m > 2).sum())
        assert open_ > 0 and rule > 0, (case, open_, rule)
    z, info = load("ctrl_corridor_sep_smooth")
    a = z["state_ctrl_actions"][:, 0]
    assert (a == 4).any() and (a != 4).any()


def test_numpy_float32_semantics_the_rules_depend_on():
    """NEP 50 (a Python int / float does not widen np.float32) and np.mean's summation order, as the device restates them."""
    assert (np.float32(2.5) + 1).dtype == np.float32
    assert np.float32(0.8) == 0.8
    rng = np.random.default_rng(1)
    for n in range(1, 33):
        for _ in range(20):
            v = (rng.random(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
            if n < 8:
                s = np.float32(0)
                for x in v:
                    s = np.float32(s + x)
            else:
                r = list(v[:8])
                i = 8
                while i < n - n % 8:
                    r = [np.float32(r[j] + v[i + j]) for j in range(8)]
                    i += 8
                s = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3])) + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
                for x in v[i:]:
                    s = np.float32(s + x)
            assert np.mean(list(v)).tobytes() == np.float32(s / np.float32(n)).tobytes()


def test_gater_requires_option2_and_separator_without_smoothing_keeps_no_buffer():
    with pytest.raises(ValueError, match="option2"):
        RuleBasedGaterAgent([], "option3", threshold_density=3)
    sep = RuleBasedSeparatorAgent(4)
    assert sep._link_inflow_buffer is None
    assert sep.take_action(np.zeros(4, np.float32)).tolist() == [2.0]
    assert sep.take_action(np.array([0, 3, 1, 1], np.float32)).tolist() == [4.0]


def test_compat_registers_the_rule_based_module():
    import pednstream_amd.compat as compat

    saved = {k: sys.modules[k] for k in list(sys.modules) if k == "rl" or k.startswith("rl.")}
    try:
        compat.install(force=True)
        from rl.agents.rule_based import RuleBasedGaterAgent as G, RuleBasedSeparatorAgent as S

        assert G is RuleBasedGaterAgent and S is RuleBasedSeparatorAgent
    finally:
        for k in [k for k in sys.modules if k == "rl" or k.startswith("rl.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def reference_statistics(agent_ids, sums):
    """rl/rl_utils.py:1650-1750 restated over recorded episode sums (np.float32 per agent and run)."""
    total_rewards, avg_rewards, per_agent = [], [], {a: [] for a in agent_ids}
    for row in sums:
        ep = {a: np.float32(row[k]) for k, a in enumerate(agent_ids)}
        total_rewards.append(sum(ep.values()))
        avg_rewards.append(np.mean(list(ep.values())))
        for a in agent_ids:
            per_agent[a].append(ep[a])
    n = len(sums)
    return {"episode_rewards": {a: np.mean(r) for a, r in per_agent.items()},
            "episode_rewards_std": {a: np.std(r) for a, r in per_agent.items()} if n > 1 else {a: 0.0 for a in agent_ids},
            "avg_reward": np.mean(avg_rewards), "avg_reward_std": np.std(avg_rewards) if n > 1 else 0.0,
            "total_reward": np.mean(total_rewards), "total_reward_std": np.std(total_rewards) if n > 1 else 0.0}


@pytest.mark.parametrize("case,runs", [("ctrl_nine_gate3", 1), ("ctrl_nine_gate3", 7), ("ctrl_one_gate3", 40), ("ctrl_small_gate08", 3)])
def test_statistics_over_runs_are_the_references(case, runs):
    z, info = load(case)
    ids = [a["id"] for a in info["rl"]["agents"]]
    sums = z["state_ctrl_episode_sums"][-runs:]          # recorded float32 sums standing in for runs
    mine = summarize_runs(ids, sums)
    ref = reference_statistics(ids, sums)
    for k, v in ref.items():
        if isinstance(v, dict):
            for a in ids:
                assert np.asarray(mine[k][a]).tobytes() == np.asarray(v[a]).tobytes(), (k, a)
        else:
            assert np.asarray(mine[k]).tobytes() == np.asarray(v).tobytes(), k
    assert len(mine["all_runs"]) == runs
    assert mine["all_runs"][0]["total_reward"] == sum(np.float32(x) for x in sums[0])


def test_evaluate_agents_refusals():
    gate = RuleBasedGaterAgent([types.SimpleNamespace(link_id="1_2", width=4)], "option2")
    with pytest.raises(ValueError, match="delta_actions"):
        evaluate_agents(None, {"gate_1": gate}, delta_actions=True)
    with pytest.raises(ValueError, match="save_dir"):
        evaluate_agents(None, {"gate_1": gate}, save_dir="out")
    with pytest.raises(TypeError, match="capture"):
        evaluate_agents(None, {"gate_1": object()})
    with pytest.raises(TypeError, match="VecPedNetEnv"):
        evaluate_agents(object(), {"gate_1": gate})


def test_header_and_exports_carry_the_controller_entries():
    from pednstream_amd import engine

    text = open(os.path.join(ROOT, "include", "pedn.h")).read()
    names = ["pedn_ctrl_configure", "pedn_ctrl_observe", "pedn_ctrl_step", "pedn_ctrl_read", "pedn_ctrl_device_ptr"]
    for n in names:
        assert re.search(r"\b" + n + r"\(", text), n
        assert n in engine.EXPORTS, n
    assert engine.ABI_VERSION == 4


def test_controller_kernels_have_no_scratch_and_fit_their_budgets(tmp_path):
    from test_kernel_resources import kernel_metadata

    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("ctrl_")}
    assert set(mine) == {f"ctrl_observe_kernel<{h}>" for h in ("true", "false")} | \
        {f"ctrl_link_turn_kernel<{p}, {h}>" for p in ("true", "false") for h in ("true", "false")}, sorted(mine)
    for name, k in mine.items():
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0, (name, k)
        if name.startswith("ctrl_observe"):
            assert k.get("sgpr_spill_count", 0) == 0, (name, k)
        else:   # the occupancy of the link_turn_kernel it stands in for: 4 waves per SIMD, 4 workgroups per CU; scalar spills go to
            # VGPR lanes (v_writelane / v_readlane), as in link_turn_kernel itself -- no memory access
            assert k["vgpr_count"] <= 128 and k["group_segment_fixed_size"] <= 40960, (name, k)
            assert k.get("sgpr_spill_count", 0) <= 32, (name, k)
