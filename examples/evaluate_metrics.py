"""Judge an ensemble: a seeded Monte-Carlo ensemble of the Delft network (every replica its own random numbers and its own Poisson
demand series), stepped through the whole horizon, then the reference's evaluation metrics (rl/rl_utils.py) of EVERY replica computed
on the device -- no history leaves the GPU -- and their distribution over the ensemble: served-trip rate and total delay.

    python examples/evaluate_metrics.py [n_replicas]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pednstream_amd import NetworkEnvGenerator  # noqa: E402
from pednstream_amd.metrics import network_metrics, replica  # noqa: E402


def main():
    R = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    np.random.seed(0)
    net = NetworkEnvGenerator(os.path.join(ROOT, "data")).create_network("delft", verbose=False, n_replicas=R, rng_seed=0)
    T = net.simulation_steps
    for nid in net.origin_nodes:                  # every replica: a Poisson realisation of the scenario's demand profile
        base = np.maximum(np.asarray(net.nodes[nid].demand, dtype=np.float64)[:T], 0.0)
        net.set_demand_matrix(nid, np.stack([np.random.default_rng(r).poisson(base).astype(np.float64) for r in range(R)]))
    net.run(1, T + 1)                             # every step up to t = T: row T holds the final cumulative flows the metrics read
    m = network_metrics(net)
    served = m["served_trips_rate"]["served_trips_rate"]
    delay = m["total_network_delay"]["total_delay"]
    q = lambda a: " / ".join(f"{v:.4g}" for v in np.percentile(a, [5, 50, 95]))
    print(f"delft x {R} replicas, {T} steps")
    print(f"served-trip rate      5 / 50 / 95 %: {q(served)}   (mean {served.mean():.4f})")
    print(f"total delay [ped s]   5 / 50 / 95 %: {q(delay)}")
    print(f"delay intensity       5 / 50 / 95 %: {q(m['total_network_delay']['delay_intensity'])}")
    print(f"congested link-steps  5 / 50 / 95 %: {q(m['network_congestion']['congestion_fraction'])}")
    worst = int(np.argmax(delay))
    print(f"worst replica {worst}: {replica(m, worst)['average_travel_time_spent']}")
    net.close()


if __name__ == "__main__":
    main()
