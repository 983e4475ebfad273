"""Shared by test_wide_agents_host.py (CPU) and test_gpu_wide_agents.py (GPU): inputs that take the RL kernels where no scenario under
data/ does -- a gater with 8 outgoing links (the second pass of rl_observe_body's per-wave link loop, LDS rows 4..7, NumPy's pairwise
summation from 8 values on) and separator controllers whose moving-average window is not 5.

hub8          a hub (node 0) with 8 spokes, each ending in a leaf; three leaves are origins, four are destinations, the last spoke lies on
              no route and stays empty.  The hub carries the one gater agent, links 0_1 .. 0_8.
SequentialSum RlOracle with the reward's two means summed left to right in float32 -- what the observation kernel did before it used
              NumPy's order.  Only there to prove that the inputs tell the two orders apart.
corridor_*    long_corridor with sparse demand (tests/sparse_demand.py), which makes the forward link's outflow -- the one value the
              separator rule reads -- exactly 0.0 for stretches shorter and longer than every tested window."""
import copy
import functools

import numpy as np

import sparse_demand as sd
from golden_util import DATA
from pednstream_amd import Network, NetworkEnvGenerator
from pednstream_amd.flatten import flatten_network
from rl_oracle import RlOracle

# Chosen so that the conditions of test_wide_agents_host.py hold.  Short links: the 16 travel times the reward sums stay near 100, where
# a float32 ulp is 8e-6, so that a last-bit change of the mean deviation (times 10) often moves the reward.  The product length * width
# is no power of two (at 8 x 4 every density is a multiple of 1/32 and all the sums are exact), and the demand keeps most densities under 4.
HUB_LENGTH, HUB_WIDTH, HUB_DEMAND, HUB_UNIT_TIME, HUB_STEPS = 6.0, 2.0, 3.0, 4.0, 260
# the controller cases: more demand and narrow exits, so that the hub's mean density crosses 2 although one spoke is empty
HUB_CTRL = {"demand": 9.0, "exit_width": 0.5}
HUB_SEED = 5
HUB_ORIGINS, HUB_DESTINATIONS = [9, 11, 14], [10, 12, 13, 15]          # leaf 16 (spoke 8) is neither: link 0_8 stays empty
HUB_LINKS = [f"0_{k}" for k in range(1, 9)]


def hub8(demand=HUB_DEMAND, length=HUB_LENGTH, width=HUB_WIDTH, unit_time=HUB_UNIT_TIME, steps=HUB_STEPS, exit_width=None):
    """(adjacency, params, origins, destinations): hub 0 -- spokes 1..8 -- leaves 9..16.  exit_width: width of the links between a
    destination leaf and its spoke (default: `width`); narrow exits make the queues spill back onto the hub's links."""
    n = 17
    adj = np.zeros((n, n), dtype=int)
    for k in range(1, 9):
        adj[0, k] = adj[k, 0] = 1
        adj[k, k + 8] = adj[k + 8, k] = 1
    params = {"unit_time": unit_time, "simulation_steps": steps, "assign_flows_type": "classic", "seed": HUB_SEED,
              "path_finder": {"k_paths": 2, "temp": 4.0, "alpha": 1.0, "beta": 0.6, "omega": 0.7},
              "default_link": {"length": length, "width": width, "free_flow_speed": 1.3, "k_critical": 1.8, "k_jam": 5.5, "gamma": 0.01,
                               "speed_noise_std": 0.04, "fd_type": "yperman", "bi_factor": 1, "activity_probability": 0.1},
              "links": {"0_3": {"width": 0.6 * width, "k_critical": 1.5}, "0_5": {"length": 1.25 * length, "k_critical": 2.1}},
              "demand": {f"origin_{o}": {"peak_lambda": demand * f, "base_lambda": 0.4 * demand * f}
                         for o, f in zip(HUB_ORIGINS, (1.0, 0.8, 0.6))},
              "controllers": {"enabled": True, "nodes": [0]}}
    if exit_width is not None:
        for d in HUB_DESTINATIONS:
            params["links"][f"{d - 8}_{d}"] = {"width": exit_width}
    return adj, params, list(HUB_ORIGINS), list(HUB_DESTINATIONS)


def hub8_network(B=1, replica_offset=0, demand=HUB_DEMAND, exit_width=None, **kw):
    adj, params, origins, dests = hub8(demand=demand, exit_width=exit_width)
    np.random.seed(HUB_SEED)
    return Network(adj, copy.deepcopy(params), origin_nodes=origins, destination_nodes=dests, verbose=False, n_replicas=B,
                   rng_seed=HUB_SEED, replica_offset=replica_offset, **kw)


HUB_SPEC = [{"id": "gate_0", "type": "gate", "links": HUB_LINKS}]


class SequentialSum(RlOracle):
    @staticmethod
    def mean(v):
        s = np.float32(0)
        for x in np.asarray(v, dtype=np.float32):
            s = np.float32(s + x)
        return np.float32(s / np.float32(len(v)))


def hub8_actions(tag, B, steps, n_actions=8, width=HUB_WIDTH):
    """[steps, B, n_actions] float32, uniform in [-0.5, width + 0.5] (outside the bounds too); row r is replica r's whatever B is"""
    return np.stack([np.random.default_rng([77, tag, r]).uniform(-0.5, width + 0.5, size=(steps, n_actions)).astype(np.float32)
                     for r in range(B)], axis=1)


# The reward-mean replicas: a batch of 16 at this replica offset, all checked, 120 env steps at action_gap 1 and 2
REWARD_OFFSET, REWARD_B, REWARD_STEPS = 1000, 16, 120


@functools.lru_cache(maxsize=None)
def reward_models(gap):
    """RlOracle and SequentialSum over the reward-mean replicas: (actions [steps, B, 8], obs [steps, B, 32], rewards [steps, B, 1] of the
    reference order, rewards of the sequential order, hub mean density per (step, B) in both orders)."""
    net = hub8_network()
    model = flatten_network(net)
    acts = hub8_actions(100 + gap, REWARD_B, REWARD_STEPS)
    out = [[], [], []]
    for r in range(REWARD_B):
        both = [cls(net, model, HUB_SPEC, "option2", False, gap, seed=HUB_SEED, replica=REWARD_OFFSET + r, reward_mode="all")
                for cls in (RlOracle, SequentialSum)]
        rows = [[m.step(acts[k, r]) for k in range(REWARD_STEPS)] for m in both]
        assert all(m.o.flags() == 0 for m in both)
        assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(*rows))
        out[0].append([o for o, _ in rows[0]])
        out[1].append([w for _, w in rows[0]])
        out[2].append([w for _, w in rows[1]])
    net.close()
    obs, rew, seq = (np.array(x).swapaxes(0, 1) for x in out)
    for a in (acts, obs, rew, seq):
        a.setflags(write=False)
    return acts, obs, rew, seq


# ---------------------------------------------------------------------------------------------------------------- separator windows
WINDOWS = (1, 8, 13, 32)
CORRIDOR_PATTERN = "drain_refill"


def corridor_network(B, replica_offset=0, **kw):
    np.random.seed(7)
    return NetworkEnvGenerator(DATA).create_network("long_corridor", verbose=False, n_replicas=B, rng_seed=HUB_SEED,
                                                    replica_offset=replica_offset, **kw)


CORRIDOR_SILENCES = (6, 12, 20, 28, 45)     # steps without demand between two pulses; the corridor smears a pulse over a few more steps
CORRIDOR_STEPS = 200                        # env steps per episode of the window tests: the train and a long silence behind it


def corridor_demand(net, B):
    """{origin: [B, T]}: a train of drain_refill's pulses (tests/sparse_demand.py: 3 steps, Poisson per replica) with CORRIDOR_SILENCES in
    between and nothing behind the last one"""
    T = int(net.simulation_steps)
    out = {}
    for k, nid in enumerate(net.origin_nodes):
        d = np.zeros((B, T))
        t = 1
        for j, silence in enumerate(CORRIDOR_SILENCES + (0,)):
            d[:, t:t + sd.DRAIN_PULSE] = sd.drain_refill(T, B, key=31 * k + j)[:, 1:1 + sd.DRAIN_PULSE]
            t += sd.DRAIN_PULSE + silence
        out[nid] = d
    return out


CORRIDOR_CHECKED = {70: (0, 63, 64, 69), 320: (0, 127, 128, 255, 256, 319)}     # batch size: the replicas whose every action is compared
CORRIDOR_SPEC = [{"id": "sep_2_3", "type": "sep", "links": ["2_3", "3_2"]}]


def separator_agent(window, width=4):
    """the reference's rule with a moving average over `window` values (pednstream_amd.agents); window None: no smoothing"""
    from pednstream_amd.agents import RuleBasedSeparatorAgent

    return RuleBasedSeparatorAgent(width, use_smoothing=window is not None, buffer_size=window or 5)


@functools.lru_cache(maxsize=None)
def corridor_series(window, r, steps=CORRIDOR_STEPS):
    """Replica r of the sparse corridor under the host agent of `window`, on the CPU oracle: (x [steps] float32, the forward link's outflow
    obs[1] after every env step; actions [steps] float32, actions[k] the one applied before step k)"""
    net = corridor_network(1)
    model = flatten_network(net)
    o = RlOracle(net, model, CORRIDOR_SPEC, "option2", False, 1, seed=HUB_SEED, replica=r)
    for nid, rows in corridor_demand(net, r + 1).items():
        o.o.set_demand(net.nodes[nid].index, rows[r])
    agent = separator_agent(window)
    obs = np.zeros(4, np.float32)
    x, acts = [], []
    for _ in range(steps):
        a = agent.take_action(obs, deterministic=True)
        acts.append(a[0])
        obs, _ = o.step(a)
        x.append(obs[1])
    assert o.o.flags() == 0
    net.close()
    return np.float32(x), np.float32(acts)
