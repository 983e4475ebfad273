"""Record the reference's evaluation metrics (rl/rl_utils.py:770-1512) for a few golden cases: tests/golden/metrics_<case>.json.

Needs the reference tree (PEDN_REFERENCE_ROOT).  For each case the reference is run again with the parameters its golden recorded
(oracle/ref_harness.py), the run is checked against the golden's arrays (or per-step digests for the full-horizon pins), saved with the
reference's own OutputHandler, and the reference's compute_* functions are called on that directory.  Their return dicts go to the
fixture verbatim (data only); a function that raises is recorded as {"error": "<type>: <message>"}.

    python tools/gen_metric_goldens.py [case ...]
"""
import hashlib
import importlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402  (sets numpy's dispatch before numpy is imported)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
# case -> reference dataset whose controllers compute_agent_local_metrics looks up (None: the case has no agents)
CASES = {"output_six_node": None, "output_corridor": "long_corridor", "six_node_full": None, "butterfly_scA_full": "butterfly_scA",
         "i45_full": "45_intersections", "delft_full": None, "melbourne_full": None,
         # the same runs continued through the last time index T: the reference's loops stop at T - 1, so row T -- the one
         # throughput and served-trip rate read -- is written only here
         "six_node_full_through_T": None, "delft_full_through_T": None}
THROUGH_T = "_through_T"


def step_digests(arr):
    a = np.ascontiguousarray(arr.T)
    return np.array([int.from_bytes(hashlib.blake2b(a[t].tobytes(), digest_size=8).digest(), "little") for t in range(a.shape[0])],
                    dtype=np.uint64)


def mutator(muts):
    def mutate(net, t):
        for (mt, kind, u, v, val) in muts:
            if mt == t:
                if kind == "back_gate_delta":
                    net.links[(u, v)].back_gate_width += val
                elif kind == "back_gate_set":
                    net.links[(u, v)].back_gate_width = val
                elif kind == "separator_set":
                    net.links[(u, v)].separator_width = val
                else:
                    raise ValueError(kind)
    return mutate if muts else None


def rerun(case):
    through_t = case.endswith(THROUGH_T)
    case = case[:-len(THROUGH_T)] if through_t else case
    z = np.load(os.path.join(GOLDEN, case + ".npz"))
    info = json.loads(str(z["info_json"]))
    assert info["scenario"] is not None, case
    net, _, state, extras = rh.run_reference(info["scenario"], seed=info["seed"], replica=info["replica"], mode=info["mode"],
                                             mutate=mutator([tuple(m) for m in info.get("mutations", [])]), np_seed=info["np_seed"])
    assert extras["steps_run"] == info["steps_run"], case
    checked = 0
    for name, arr in state.items():
        if info.get("digest"):
            if "state_digest_" + name in z.files:
                assert np.array_equal(step_digests(arr), z["state_digest_" + name]), (case, name)
                checked += 1
        elif "state_" + name in z.files:
            ref = z["state_" + name]
            assert arr.shape == ref.shape and np.array_equal(arr, ref, equal_nan=True), (case, name)
            checked += 1
    assert checked >= 13, (case, checked)
    if through_t:
        T = net.simulation_steps
        assert info["steps_run"] == T and not info.get("mutations"), case
        with rh.InjectedRNG(net, seed=info["seed"], replica=info["replica"], mode=info["mode"]):
            net.network_loading(T)
        info = dict(info, steps_run=T + 1)
    return net, info


def call(fn, **kw):
    try:
        return fn(**kw)
    except (ValueError, KeyError) as err:
        return {"error": f"{type(err).__name__}: {err}"}


def metrics_of(net, dataset):
    rh.load_reference_rl()     # a bare `rl` package (its __init__ needs pettingzoo): rl.rl_utils imports under it
    utils = importlib.import_module("rl.rl_utils")
    if rh.REF_ROOT not in sys.path:
        sys.path.insert(0, rh.REF_ROOT)
    from handlers.output_handler import OutputHandler

    with tempfile.TemporaryDirectory() as tmp:
        OutputHandler(base_dir=tmp, simulation_dir="run").save_network_state(net)
        d = os.path.join(tmp, "run")
        res = {"network_throughput": call(utils.compute_network_throughput, simulation_dir=d),
               "served_trips_rate": call(utils.compute_served_trips_rate, simulation_dir=d),
               "total_network_delay": call(utils.compute_total_network_delay, simulation_dir=d),
               "average_travel_time_spent": call(utils.compute_average_travel_time_spent, simulation_dir=d),
               "network_congestion": call(utils.compute_network_congestion_metric, simulation_dir=d),
               "network_travel_time": call(utils.compute_network_travel_time, simulation_dir=d)}
        if dataset is not None:
            # compute_agent_local_metrics calls create_network(dataset, verbose=False), a keyword the reference's own
            # NetworkEnvGenerator.create_network does not take: the call is given a wrapper that drops it (in memory only)
            gen_cls = rh.load_reference()["env"].NetworkEnvGenerator
            create = gen_cls.create_network
            gen_cls.create_network = lambda self, *a, verbose=None, **kw: create(self, *a, **kw)
            cwd = os.getcwd()
            os.chdir(rh.REF_ROOT)       # NetworkEnvGenerator() reads data/ relative to the working directory
            try:
                res["agent_local_metrics"] = utils.compute_agent_local_metrics(simulation_dir=d, dataset=dataset)
            finally:
                os.chdir(cwd)
                gen_cls.create_network = create
    return res


def plain(x):
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (np.integer, int)) and not isinstance(x, bool):
        return int(x)
    if isinstance(x, (np.floating, float)):
        return float(x)
    return x


def main(cases):
    for case in cases:
        net, info = rerun(case)
        res = plain(metrics_of(net, CASES[case]))
        out = {"case": case, "scenario": info["scenario"], "steps_run": info["steps_run"], "metrics": res}
        path = os.path.join(GOLDEN, f"metrics_{case}.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        print(f"{case}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
