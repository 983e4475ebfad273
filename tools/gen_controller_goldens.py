"""Fixtures of the rule-based controllers (tests/golden/ctrl_*.npz) from the REAL reference.  TEST INFRASTRUCTURE.

Run in the build container (needs the reference tree, see oracle/ref_harness.py):   python tools/gen_controller_goldens.py [case ...]

Modelled on oracle/gen_golden.py:rl_case: the reference's ActionApplier / ObservationBuilder / reward around network_loading
(ref_harness.RefEnvShim), driven by the reference's own rl/agents/rule_based.py the way rl/rl_utils.py:1513-1610 drives an agent
(_evaluate_single_run): the reset observation is build_observation(a, sim_step=1) (pz_pednet_env.py:184-190,256-261), then
take_action on every observation until the episode terminates, episode_true_rewards[a] = 0.0; += rewards[a].  Every fixture holds
per-step actions, observations, rewards and episode sums, and the digests of the 13 per-link arrays at every time index.
"""
import copy
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ref_harness as rh  # noqa: E402  (sets the numpy environment before numpy is imported)
from gen_golden import save, step_digests  # noqa: E402

import numpy as np  # noqa: E402

import wide_agents as wa  # noqa: E402  (the hub with 8 spokes)

NP_SEED = 20261003


def rule_based_module():
    """rl/agents/rule_based.py on its own (it imports only numpy; rl/agents/__init__ would pull in torch agents)."""
    path = os.path.join(rh.REF_ROOT, "rl", "agents", "rule_based.py")
    spec = importlib.util.spec_from_file_location("ref_rule_based", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def controller_case(case, name, obs_mode="option2", normalize=False, action_gap=1, threshold=3, smoothing=None, episodes=1,
                    seed=0, replica=0, buffer_size=5, direct=None):
    """smoothing None: gaters at `threshold`; False / True: separators without / with a moving average over `buffer_size` values.
    direct: (adjacency, params, origins, destinations) of a network built with the reference's Network itself instead of scenario
    `name` (oracle/gen_golden.py:direct_case)."""
    ref = rh.load_reference()
    rb = rule_based_module()
    agents = None
    acts, obs_l, rew_l, ep_l, episode_of = [], [], [], [], []
    reset_obs = []
    state = static = None
    for e in range(episodes):
        np.random.seed(NP_SEED)                    # the same demand every episode (a reset without randomisation)
        if direct is None:
            net = ref["env"].NetworkEnvGenerator().create_network(name)
        else:
            adj, params, origins, dests = direct
            net = ref["network"].Network(np.array(adj), copy.deepcopy(params), origin_nodes=list(origins), destination_nodes=list(dests))
        if static is None:
            static = rh.dump_static(net)
        env = rh.RefEnvShim(net, obs_mode=obs_mode, normalize_obs=normalize, action_gap=action_gap)
        am = env.agent_manager
        ids = env.possible_agents
        if agents is None:                          # created once: a separator's buffer survives the reset
            agents = {}
            for a in ids:
                if am.get_agent_type(a) == "sep":
                    if smoothing is not None:
                        agents[a] = rb.RuleBasedSeparatorAgent(am.get_separator_links(a)[0].width, use_smoothing=smoothing, buffer_size=buffer_size)
                elif smoothing is None:
                    agents[a] = rb.RuleBasedGaterAgent(am.get_gater_outgoing_links(a), obs_mode, threshold_density=threshold)
            spec = []
            for a in ids:
                if am.get_agent_type(a) == "sep":
                    f, r = am.get_separator_links(a)
                    spec.append({"id": a, "type": "sep", "links": [f.link_id, r.link_id]})
                else:
                    spec.append({"id": a, "type": "gate", "links": [l.link_id for l in am.get_gater_outgoing_links(a)]})
        else:                                        # the gaters read their links off the new network (as rl/train_rl.py rebuilds them)
            for a in ids:
                if a in agents and isinstance(agents[a], rb.RuleBasedGaterAgent):
                    agents[a].outgoing_links = am.get_gater_outgoing_links(a)
        obs = {a: env.obs_builder.build_observation(a, env.sim_step) for a in ids}
        reset_obs.append(np.concatenate([np.asarray(obs[a], dtype=np.float32) for a in ids]))
        ep = {a: 0.0 for a in ids}
        with rh.InjectedRNG(net, seed=seed, replica=replica):
            done = False
            while not done:
                actions, row = {}, []
                for a in ids:
                    if a in agents:
                        act = agents[a].take_action(obs[a], deterministic=True)
                        actions[a] = act
                        row.extend(np.asarray(act, dtype=np.float32).tolist())
                    else:
                        n = 1 if am.get_agent_type(a) == "sep" else len(am.get_gater_outgoing_links(a))
                        row.extend([float("nan")] * n)
                obs, rew, term = env.step(actions)
                for a in ids:
                    ep[a] += rew[a]
                acts.append(row)
                obs_l.append(np.concatenate([np.asarray(obs[a], dtype=np.float32) for a in ids]))
                rew_l.append([np.float32(rew[a]) for a in ids])
                ep_l.append([np.float32(ep[a]) for a in ids])
                episode_of.append(e)
                done = any(term.values())
        steps_run = env.sim_step
        state = rh.dump_state(net, steps=steps_run)   # (the last episode's histories)
    payload = {"digest_" + k: step_digests(v[:, :steps_run]) for k, v in state.items() if not k.startswith("v")}
    payload.update({
        "ctrl_actions": np.array(acts, dtype=np.float32), "ctrl_obs": np.array(obs_l, dtype=np.float32),
        "ctrl_rewards": np.array(rew_l, dtype=np.float32), "ctrl_episode_sums": np.array(ep_l, dtype=np.float32),
        "ctrl_episode": np.array(episode_of, dtype=np.int32), "ctrl_reset_obs": np.array(reset_obs, dtype=np.float32)})
    controllers = {a: ({"kind": "gate", "threshold": threshold, "widths": [l.width for l in ag.outgoing_links]}
                       if isinstance(ag, rb.RuleBasedGaterAgent) else
                       {"kind": "sep", "width": ag.road_width, "use_smoothing": ag.use_smoothing, "buffer_size": ag.buffer_size})
                   for a, ag in agents.items()}
    where = {"scenario": name} if direct is None else {
        "scenario": None, "adjacency": np.array(direct[0]).tolist(), "params": direct[1], "origin_nodes": list(direct[2]),
        "destination_nodes": list(direct[3]), "tf_nodes": [], "tf_values": []}
    info = {**where, "seed": seed, "replica": replica, "mode": "philox", "np_seed": NP_SEED, "mutations": [],
            "rl": {"obs_mode": obs_mode, "normalize": normalize, "action_gap": action_gap, "agents": spec},
            "controllers": controllers, "episodes": episodes, "env_steps": len(acts) // episodes}
    save(case, static, payload, {"draws": {}, "steps_run": steps_run}, info)


CASES = {
    "ctrl_nine_gate3": lambda: controller_case("ctrl_nine_gate3", "nine_intersections", threshold=3),
    "ctrl_one_gate3": lambda: controller_case("ctrl_one_gate3", "one_intersection_v0", threshold=3),
    "ctrl_small_gate08": lambda: controller_case("ctrl_small_gate08", "small_network", threshold=0.8),
    "ctrl_nine_gate3_g2n": lambda: controller_case("ctrl_nine_gate3_g2n", "nine_intersections", threshold=3, action_gap=2, normalize=True),
    "ctrl_corridor_sep": lambda: controller_case("ctrl_corridor_sep", "long_corridor", smoothing=False),
    "ctrl_corridor_sep_smooth": lambda: controller_case("ctrl_corridor_sep_smooth", "long_corridor", smoothing=True),
    "ctrl_corridor_sep_smooth_2ep": lambda: controller_case("ctrl_corridor_sep_smooth_2ep", "long_corridor", smoothing=True, episodes=2),
    "ctrl_hub8_gate": lambda: controller_case("ctrl_hub8_gate", None, threshold=3, direct=wa.hub8(**wa.HUB_CTRL)),
    "ctrl_hub8_gate0": lambda: controller_case("ctrl_hub8_gate0", None, threshold=0.0, direct=wa.hub8(**wa.HUB_CTRL)),
    "ctrl_corridor_sep_w1": lambda: controller_case("ctrl_corridor_sep_w1", "long_corridor", smoothing=True, buffer_size=1),
    "ctrl_corridor_sep_w8": lambda: controller_case("ctrl_corridor_sep_w8", "long_corridor", smoothing=True, buffer_size=8),
    "ctrl_corridor_sep_w13": lambda: controller_case("ctrl_corridor_sep_w13", "long_corridor", smoothing=True, buffer_size=13, episodes=2),
    "ctrl_corridor_sep_w32": lambda: controller_case("ctrl_corridor_sep_w32", "long_corridor", smoothing=True, buffer_size=32),
}

if __name__ == "__main__":
    for c in sys.argv[1:] or list(CASES):
        CASES[c]()
