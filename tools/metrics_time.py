"""Time the evaluation metrics of melbourne x 1024 over the whole window (T + 1 = 501 rows) on the device against the host route
(read_field of travel_time / num_pedestrians / density and of the row-T cumulative flows, then every metric of every replica in numpy),
and report the accumulate kernel's bytes over its time (the three fields alone, and with the accumulators).  --rl: the per-step cost
of VecPedNetEnv(track_metrics=True) on 45_intersections x 2048.  The kernel times are HIP events around the launch on the engine's stream (timer_begin / timer_end), best and median of
`--reps` calls after one warm-up call.

    python tools/metrics_time.py [--replicas 1024] [--reps 10] [--no-host] [--rl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pednstream_amd import NetworkEnvGenerator  # noqa: E402
from pednstream_amd import metrics as pm  # noqa: E402


def rl_tracking_cost(n_envs, steps, history):
    """45_intersections x n_envs, env steps without a fetch (action_gap 1): host clock over `steps` steps after 50 of warm-up, ending
    in a synchronise, with metric tracking off and on, alternated three times; best of each."""
    from pednstream_amd.rl_env import VecPedNetEnv

    res = {"off": [], "on": []}
    for _ in range(3):
        for mode in ("off", "on"):
            np.random.seed(7)
            env = VecPedNetEnv("45_intersections", n_envs, data_dir=os.path.join(ROOT, "data"), seed=1, track_metrics=(mode == "on"),
                               history=history)
            env.reset()
            for _ in range(50):
                env.step(None, fetch=False)
            e = env.network.engine()
            e.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                env.step(None, fetch=False)
            e.synchronize()
            res[mode].append((time.perf_counter() - t0) / steps * 1e6)
            env.close()
    return {f"rl_{history}_workload": f"45_intersections x {n_envs} envs, history={history!r}, {steps} env steps, no fetch",
            f"rl_{history}_us_per_step_tracking_off": round(min(res["off"]), 1),
            f"rl_{history}_us_per_step_tracking_on": round(min(res["on"]), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--rl", action="store_true", help="also: the per-step cost of VecPedNetEnv(track_metrics=True)")
    ap.add_argument("--rl-envs", type=int, default=2048)
    ap.add_argument("--rl-steps", type=int, default=300)
    args = ap.parse_args()
    R = args.replicas
    np.random.seed(7)
    net = NetworkEnvGenerator(os.path.join(ROOT, "data")).create_network("melbourne", verbose=False, n_replicas=R, rng_seed=5)
    T1 = net.simulation_steps + 1
    net.run(1, T1)
    e = net.engine()
    e.synchronize()
    em = pm.EpisodeMetrics(net)
    kernel, call = [], []
    for k in range(args.reps + 1):
        em.restart()
        e.synchronize()
        t0 = time.perf_counter()
        e.timer_begin()
        em.add(0, T1)
        ms = e.timer_end()                      # synchronises
        res = em.result()
        t1 = time.perf_counter()
        if k:
            kernel.append(ms)
            call.append((t1 - t0) * 1e3)
    L = net.n_links
    field_bytes = 3 * 4 * T1 * L * R            # the three f32 fields, every row, every (link, replica)
    acc_bytes = 2 * 11 * 8 * L * e.n_replicas   # accumulators read and written once
    best, med = min(kernel), float(np.median(kernel))
    out = {"workload": f"melbourne x {R}, {L} links, {T1} rows", "field_bytes": field_bytes, "accumulator_bytes": acc_bytes,
           "accumulate_ms_best": round(best, 3), "accumulate_ms_median": round(med, 3),
           "accumulate_TBps_best_field_bytes": round(field_bytes / best / 1e9, 2),
           "accumulate_TBps_best_all_bytes": round((field_bytes + acc_bytes) / best / 1e9, 2),
           "call_ms_median": round(float(np.median(call)), 3),
           "served_trips_rate_mean": float(np.mean(res["served_trips_rate"]["served_trips_rate"])),
           "total_delay_mean": float(np.mean(res["total_network_delay"]["total_delay"]))}
    if not args.no_host:
        # the host route: the three fields and the row-T cumulative flows copied off the device (Network.read_field), then every metric
        # of every replica in numpy (tests/metrics_model.batched_metrics: the same per-row terms and folds as the device path)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import metrics_model as mm

        t0 = time.perf_counter()
        tt, n, d = (net.read_field(f) for f in ("travel_time", "num_pedestrians", "density"))
        ci = net.read_field("cumulative_inflow", T1 - 1, T1)[0, :L]
        co = net.read_field("cumulative_outflow", T1 - 1, T1)[0, :L]
        t1 = time.perf_counter()
        dem = 0.0
        for nid in net.origin_nodes:          # every replica runs the scenario's demand here
            s_ = 0.0
            for x in net.nodes[nid].demand:
                s_ += float(x)
            dem += s_
        host = {}
        for r0 in range(0, R, 64):
            r1 = min(R, r0 + 64)
            part, _ = mm.batched_metrics(net, tt[:, :L, r0:r1], n[:, :L, r0:r1], d[:, :L, r0:r1], ci[:, r0:r1], co[:, r0:r1],
                                         np.full(r1 - r0, dem))
            for name, dd in part.items():
                for k, v in dd.items():
                    host.setdefault(name, {}).setdefault(k, []).append(v)
        t2 = time.perf_counter()
        worst = 0.0
        for name, dd in host.items():
            for k, parts in dd.items():
                h, g = np.concatenate(parts).astype(np.float64), res[name][k].astype(np.float64)
                worst = max(worst, float(np.max(np.abs(h - g) / np.maximum(np.abs(h), 1e-300))))
        out.update({"host_read_field_ms": round((t1 - t0) * 1e3, 1), "host_numpy_ms": round((t2 - t1) * 1e3, 1),
                    "host_total_ms": round((t2 - t0) * 1e3, 1), "host_vs_device_max_rel_diff": worst})
    if args.rl:
        for history in ("full", "recent"):
            out.update(rl_tracking_cost(args.rl_envs, args.rl_steps, history))
    net.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
