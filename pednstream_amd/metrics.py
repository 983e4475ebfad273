"""The reference's evaluation metrics for every replica, computed on the device.

Mirrors rl/rl_utils.py:770-1512 of the reference: ``compute_network_throughput``, ``compute_served_trips_rate``,
``compute_total_network_delay``, ``compute_average_travel_time_spent``, ``compute_network_congestion_metric``,
``compute_network_travel_time`` and ``compute_agent_local_metrics``.  The reference computes them from the JSON that
``OutputHandler.save_network_state`` writes; here replica ``r`` gets what those functions return for the directory
``OutputHandler.save_network_state(network, replica=r)`` would write at that moment, without any history leaving the device
(include/pedn.h: pedn_metrics_*).

Counts and the short serial sums (demand, row-T cumulative flows) are exactly the reference's.  Sums over (link, time) are
per-link serial partial sums folded in link order: they differ from the reference's one serial sum by rounding only, and they
are bit-identical from run to run, for any batch size or launch plan, and for any split of the rows into consecutive windows.

There is no CPU fallback: the numbers come from the HIP engine or the call fails.
"""
import numpy as np

# index in the rows of pedn_metrics_read (include/pedn.h: PEDN_M_*)
_M = {name: i for i, name in enumerate((
    "throughput", "completed_demand", "total_demand",
    "avg_travel_time", "tt_num_links",
    "total_delay", "delay_intensity", "delay_person_time", "delay_num_links",
    "avg_travel_time_spent", "person_time", "total_trips", "num_origin_links",
    "served_trips_rate", "total_inflow", "total_outflow", "num_destination_links",
    "congestion_time", "avg_congestion_density", "congestion_fraction", "total_area_time",
    "congested_rows", "counted_rows"))}

# metric name -> [(key of the reference's return dict, row of pedn_metrics_read, integer?)]
LAYOUT = {
    "network_throughput": [("throughput", "throughput", False), ("completed_demand", "completed_demand", False),
                           ("total_demand", "total_demand", False), ("completion_rate", "throughput", False)],
    "served_trips_rate": [("served_trips_rate", "served_trips_rate", False), ("total_inflow", "total_inflow", False),
                          ("total_outflow", "total_outflow", False), ("num_origin_links", "num_origin_links", True),
                          ("num_destination_links", "num_destination_links", True)],
    "total_network_delay": [("total_delay", "total_delay", False), ("delay_intensity", "delay_intensity", False),
                            ("total_person_time", "delay_person_time", False), ("num_links", "delay_num_links", True)],
    "average_travel_time_spent": [("avg_travel_time_spent", "avg_travel_time_spent", False),
                                  ("total_person_time", "person_time", False), ("total_trips", "total_trips", False),
                                  ("num_origin_links", "num_origin_links", True)],
    "network_congestion": [("congestion_time", "congestion_time", False), ("avg_congestion_density", "avg_congestion_density", False),
                           ("congestion_fraction", "congestion_fraction", False), ("total_area_time", "total_area_time", False)],
    "network_travel_time": [("avg_travel_time", "avg_travel_time", False), ("num_links", "tt_num_links", True)],
}
# beyond the reference's keys: the row counts behind congestion_fraction
EXTRA = {"network_congestion": [("congested_rows", "congested_rows", True), ("counted_rows", "counted_rows", True)]}

_ORIGIN, _DEST, _ODPATH = 1, 2, 4


def _network_of(obj):
    return obj.network if hasattr(obj, "network") and not hasattr(obj, "links") else obj


def link_flags(network):
    """[n_links] int32: bit 0 starts at an origin node, bit 1 ends at a destination node, bit 2 lies on an od path (every link when
    the network has no path finder, or no path at all: rl_utils.py:916-936)."""
    origins, dests = set(network.origin_nodes), set(network.destination_nodes)
    od_links = set()
    pf = getattr(network, "path_finder", None)
    if pf is not None:
        for paths in pf.od_paths.values():
            for path in paths:
                od_links.update(f"{u}-{v}" for u, v in zip(path[:-1], path[1:]))
    flags = np.zeros(network.n_links, dtype=np.int32)
    for (u, v), link in network.links.items():
        f = (_ORIGIN if u in origins else 0) | (_DEST if v in dests else 0)
        if not od_links or f"{u}-{v}" in od_links:
            f |= _ODPATH
        flags[link.index] = f
    return flags


def agent_links(network):
    """(agent ids, ptr [n_agents + 1], links, link keys) as rl_env.AgentManager assigns them: a gater's real incoming then real
    outgoing links, a separator's forward and reverse link (rl_utils.py:1343-1366)."""
    from .rl_env import AgentManager

    am = AgentManager(network)
    ids, ptr, links, keys = am.get_all_agent_ids(), [0], [], []
    for aid in ids:
        if am.get_agent_type(aid) == "gate":
            node = am.get_gater_node(aid)
            mine = [l for l in node.incoming_links if not l.is_virtual] + [l for l in node.outgoing_links if not l.is_virtual]
        else:
            mine = list(am.get_separator_links(aid))
        links += [l.index for l in mine]
        keys += [f"{l.start_node.node_id}-{l.end_node.node_id}" for l in mine]
        ptr.append(len(links))
    return ids, np.array(ptr, np.int32), np.array(links, np.int32), keys


class EpisodeMetrics:
    """Accumulates the metrics of every replica of ``network`` over windows of rows ``add(t0, t1)`` (increasing, not overlapping; rows no
    window covers read as zero).  ``result()`` finalises.  One accumulator set per engine: beginning another one (a second
    ``EpisodeMetrics``, ``network_metrics``) ends this one -- except while a ``VecPedNetEnv(track_metrics=True)`` owns the set
    (``tracking``): then beginning another one is refused, so that the tracked episode is never lost."""

    def __init__(self, network, agents=False, tracking=False):
        self.network = _network_of(network)
        self._agents = agent_links(self.network) if agents else None
        self.tracking = bool(tracking)
        self.restart()

    def restart(self):
        """Accumulators back to zero (a new episode)."""
        net = self.network
        owner = getattr(net._engine, "_metrics_owner", None) if net._engine is not None else None
        if owner is not None and owner is not self and owner.tracking:
            raise RuntimeError("an env tracks the metrics of this engine (VecPedNetEnv(track_metrics=True)): read them with "
                               "env.episode_metrics() / agent_local_metrics(env); another accumulation would discard the tracked episode")
        eng = net._flush()
        rows, lens = [], []
        dem_row = eng.model["node_demand_row"]
        for nid in net.origin_nodes:
            node = net.nodes.get(nid)
            d = None if node is None else node.demand
            rows.append(-1 if node is None else int(dem_row[node.index]))
            lens.append(0 if d is None else len(d))
        ptr, links = (self._agents[1], self._agents[2]) if self._agents else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        eng.metrics_begin(link_flags(net), rows, lens, ptr, links, net.unit_time)
        eng._metrics_owner = self
        self._eng = eng

    def _check(self):
        if self.network._engine is not self._eng or getattr(self._eng, "_metrics_owner", None) is not self:
            raise RuntimeError("the engine's metric accumulators were begun again by another caller; restart() this one")

    def add(self, t0, t1=None):
        """Fold rows t0 <= t < t1 (default: t0 + 1) in.  IndexError when a row has left a field's ring (history="recent")."""
        self._check()
        self._eng.metrics_accumulate(t0, t0 + 1 if t1 is None else t1)

    def _read(self):
        self._check()
        return self._eng.metrics_read()

    def result(self):
        """{metric name: {key of the reference's dict: [n_replicas] array}}; counts are int64."""
        out, _, _ = self._read()
        return _dicts(out)

    def agent_result(self):
        """{agent id: {"avg_density", "avg_normalized_density", "num_links": [n_replicas], "link_densities",
        "link_normalized_densities": {link key: [n_replicas]}}} (compute_agent_local_metrics; NaN for a link without valid rows)."""
        if self._agents is None:
            raise RuntimeError("EpisodeMetrics(..., agents=True) is needed for agent-local metrics")
        _, al, ag = self._read()
        ids, ptr, _, keys = self._agents
        res = {}
        for a, aid in enumerate(ids):
            js = range(ptr[a], ptr[a + 1])
            res[aid] = {"avg_density": ag[:, a, 0].copy(), "avg_normalized_density": ag[:, a, 1].copy(),
                        "num_links": ag[:, a, 2].astype(np.int64),
                        "link_densities": {keys[j]: al[:, j, 0].copy() for j in js},
                        "link_normalized_densities": {keys[j]: al[:, j, 1].copy() for j in js}}
        return res


def _dicts(out):
    res = {}
    for name, keys in LAYOUT.items():
        d = {}
        for key, row, is_int in keys + EXTRA.get(name, []):
            col = out[:, _M[row]]
            d[key] = col.astype(np.int64) if is_int else col.copy()
        res[name] = d
    return res


def network_metrics(network, t0=0, t1=None):
    """One-shot metrics of every replica over rows t0 <= t < t1 (default: all T + 1 rows; rows outside read as zero, as do rows no step
    has written yet): {"network_throughput", "served_trips_rate", "total_network_delay", "average_travel_time_spent",
    "network_congestion", "network_travel_time"} -> {key: [n_replicas] array}."""
    net = _network_of(network)
    em = EpisodeMetrics(net)
    em.add(t0, net.simulation_steps + 1 if t1 is None else t1)
    return em.result()


def agent_local_metrics(env, t0=0, t1=None):
    """compute_agent_local_metrics for every replica of a ``VecPedNetEnv`` (or a Network with controllers): from the env's tracked
    episode when it tracks metrics, else one-shot over rows t0 <= t < t1."""
    if getattr(env, "_metrics", None) is not None and t0 == 0 and t1 is None:
        return env._tracked_metrics().agent_result()
    net = _network_of(env)
    em = EpisodeMetrics(net, agents=True)
    em.add(t0, net.simulation_steps + 1 if t1 is None else t1)
    return em.agent_result()


def replica(result, r):
    """The reference's plain dicts for replica ``r`` of a ``network_metrics`` / ``EpisodeMetrics.result`` result (reference keys only)
    or of an agent-local result."""
    if set(result) <= set(LAYOUT):
        return {name: {key: (int(d[key][r]) if np.issubdtype(d[key].dtype, np.integer) else float(d[key][r]))
                       for key, _, _ in LAYOUT[name]} for name, d in result.items()}
    res = {}
    for aid, d in result.items():
        ld = {k: float(v[r]) for k, v in d["link_densities"].items() if not np.isnan(v[r])}
        ln = {k: float(v[r]) for k, v in d["link_normalized_densities"].items() if not np.isnan(v[r])}
        res[aid] = {"avg_density": float(d["avg_density"][r]), "avg_normalized_density": float(d["avg_normalized_density"][r]),
                    "num_links": int(d["num_links"][r]), "link_densities": ld, "link_normalized_densities": ln}
    return res
