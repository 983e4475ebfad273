"""bench.py without a GPU: the command line the driver uses parses, the synthetic demand is a function of the replica id only
(it keys results to the GLOBAL replica id, whatever the rank count), and a WORLD_SIZE that disagrees with --gpus is refused
before anything is imported."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_help_lists_the_contract_flags():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--replicas", "--total-replicas", "--network", "--rl", "--randomize", "--history",
                 "--dump-outputs", "--full"):
        assert flag in out.stdout, flag


def test_world_size_mismatch_is_refused_early():
    env = dict(os.environ, WORLD_SIZE="4")
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode != 0 and "WORLD_SIZE" in out.stderr


def test_replica_demand_is_keyed_by_the_global_replica_id():
    sys.path.insert(0, ROOT)
    import bench

    a, b = bench.replica_demand(500, 7), bench.replica_demand(500, 7)
    assert np.array_equal(a, b) and a.dtype == np.float64 and len(a) == 500
    assert not np.array_equal(a, bench.replica_demand(500, 8))
    assert bench.BYTES_PER_LINK_UPDATE == bench.NODE_KERNEL_BYTES + bench.LINK_KERNEL_BYTES == 212


def _full_object():
    """A full bench object of the shape main() builds (every block, long prose strings where the real one has them)."""
    prose = "x" * 600
    rf = {"bound": "hbm", "kernel": prose, "kernel_name": "node_kernel<LU>", "achieved": 5441.1859, "peak": 8000.0, "unit": "GB/s", "frac": 0.68014821,
          "basis_kind": "moved", "basis": prose, "traffic": 80879083.2, "traffic_source": prose, "frac_algorithmic": 0.8562, "frac_counter": 0.6801,
          "frac_executed": 0.5931, "traffic_bytes_per_link_update": 168.4, "algorithmic_bytes_per_link_update": 212,
          "algorithmic_bytes_per_launch": 101814272, "fits_infinity_cache": True, "concurrent_chains": 2, "avg_launch_ms": 0.02592,
          "whole_step_frac": 0.8484, "whole_step_frac_counter": 0.674, "note": prose, "per_launch": {"note": prose},
          "launch_plan": {"chains": 2, "link_update_by_next_node_kernel": True, "probe": prose}, "one_chain": {"avg_launch_ms": 0.0322, "frac": 0.79, "note": prose}}
    variant = {"value": 1.9e10, "unit": "link-updates/s", "ms_per_step": 0.0435, "device_ms_per_step": 0.0434, "steps": 300, "warmup": 100,
               "config": {"workload": prose}, "roofline": dict(rf), "cpu_baseline": {"sample": prose}}
    rl = {"value": 8.1e7, "ms_per_step": 0.0252, "whole_step_frac": 0.362, "config": {"workload": prose}}
    return {"metric": "link-updates/sec (links x replicas x steps/sec)", "value": 31951388757.4, "unit": "link-updates/s", "n_gpus": 1, "ranks_seen": 1,
            "steps": 20, "warmup": 5, "ms_per_step": 0.0300616, "device_ms_per_step": 0.02999, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64+f32", "data": "synthetic",
            "config": {"workload": prose, "network": "melbourne", "history": "full-record", "replicas_per_gpu": 1024, "replicas_total": 1024, "links": 938,
                       "parallelism": prose},
            "roofline": rf,
            "cpu_baseline": {"value": 8.4e7, "unit": "link-updates/s", "cores": 256, "kind": "port", "sample": prose,
                             "sample_short": "1280 replicas x 499 steps of melbourne, 256 threads, 7.1 s; 1 thread: 54 replicas, 7.0 s", "one_thread": 3.5e6,
                             "all_cores": 8.4e7, "cpu_model": "AMD EPYC 9575F 64-Core Processor", "executed_paths": {"a": 1},
                             "reference_python_equiv": {"label": prose, "one_core": 27920.1, "all_cores": 6.6e5}},
            "extra": {"headline_long_window": dict(variant), "config3_delft_x1024": dict(variant), "hbm_proper_melbourne_x4096": dict(variant),
                      "melbourne_heavy_x1024": dict(variant), "nine_x256": dict(variant), "broken": {"error": prose},
                      "config5_rl_45int_x2048": {"plain": dict(rl), "randomized": dict(rl),
                                                 "by_n_envs_recent_history": {str(n): {"value": 1e8} for n in (1024, 2048, 4096, 8192)},
                                                 "end_to_end_random_policy": {"eager": {"value": 3.2e7}, "graph_replay": {"value": 6e7}},
                                                 "end_to_end_mlp_policy": {"eager": {"value": 1.3e7}, "graph_replay": {"value": 5e7}},
                                                 "sustained": {f"{m}_{h}": {"value": 7e7, "wall_s": 1.0} for h in ("full", "recent")
                                                               for m in ("plain", "vectorised", "reference")}}}}


def test_compact_line_is_small_and_carries_the_contract_fields():
    """the driver keeps an 8 KB tail of stdout and parses its last line -- the line must stay under 4 KB whatever the
    run measured, and carry metric / value / roofline.frac / cpu_baseline.value as numbers."""
    import json

    sys.path.insert(0, ROOT)
    import bench

    line = json.dumps(bench.compact_line(_full_object()), separators=(",", ":"))
    assert len(line) < 4096, len(line)
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "ranks_seen", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["config"]["workload"].startswith("melbourne x 1024") and "model" not in d["config"]
    rf = d["roofline"]
    for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "basis_kind", "traffic", "frac_algorithmic", "frac_counter", "frac_executed",
              "avg_launch_ms", "launch_plan"):
        assert k in rf, k
    assert rf["kernel"] == "node_kernel<LU>" and 0 < rf["frac"] < 1
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] == 256 and cb["kind"] == "port" and len(cb["sample"]) < 120
    assert d["extra"]["config5_rl_45int_x2048"]["end_to_end_mlp_policy"]["graph_replay"] == 5e7
    assert all(len(json.dumps(v)) < 900 for v in d["extra"].values())
    # no prose anywhere
    assert "xxxx" not in line.replace(d["extra"]["broken"]["error"], "")


def test_plain_line_carries_the_headline_only():
    """A plain run (no --full) measures no roofline, CPU baseline or extras: its line is the headline fields and the config, the same
    values a --full run prints for them, and names no bench_full.json."""
    sys.path.insert(0, ROOT)
    import bench

    full = _full_object()
    plain = {k: v for k, v in full.items() if k not in ("roofline", "cpu_baseline", "extra")}
    line, full_line = bench.compact_line(plain), bench.compact_line(full, "bench_full.json")
    assert set(line) == {"metric", "value", "unit", "n_gpus", "ranks_seen", "steps", "warmup", "ms_per_step", "device_ms_per_step",
                         "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}
    assert full_line["full"] == "bench_full.json" and "roofline" in full_line and "cpu_baseline" in full_line and "extra" in full_line
    for k in line:
        assert line[k] == full_line[k], k


def test_dump_outputs_is_refused_where_it_is_not_supported(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE"):
        env.pop(k, None)
    for extra in (["--gpus", "2"], ["--rl"]):
        out = subprocess.run([sys.executable, BENCH, "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / "d")] + extra,
                             capture_output=True, text=True, env=env, timeout=120)
        assert out.returncode != 0 and "--dump-outputs" in out.stderr, extra
    assert not (tmp_path / "d").exists()


class _FakeEngine:
    """read_block of a known pattern: value = field * 1e6 + row * 1e3 + column + replica / 1e4."""

    def __init__(self, n_links, n_vlinks, n_replicas):
        self.n_links, self.n_all, self.n_replicas = n_links, n_links + n_vlinks, n_replicas

    def read_block(self, field, t0, t1):
        cols = self.n_all if field < 4 else self.n_links
        t, c, r = np.meshgrid(np.arange(t0, t1), np.arange(cols), np.arange(self.n_replicas), indexing="ij")
        return (field * 1e6 + t * 1e3 + c + r / 1e4).astype(np.float64 if field < 7 else np.float32)


@pytest.mark.parametrize("n_links, n_replicas", [(24, 64), (938, 1024)])
def test_dump_outputs_writes_the_last_step_within_the_budget(tmp_path, n_links, n_replicas):
    sys.path.insert(0, ROOT)
    import bench
    from pednstream_amd.network import LINK_FIELDS

    e, t = _FakeEngine(n_links, 9, n_replicas), 25
    bench.dump_outputs(e, t, str(tmp_path / "a"), offset=100)
    bench.dump_outputs(e, t, str(tmp_path / "b"), offset=100)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted([f + ".npy" for f in LINK_FIELDS] + ["replicas.npy"])
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10 ** 6
    reps = np.load(tmp_path / "a" / "replicas.npy")
    assert reps.dtype == np.float64 and np.all(np.diff(reps) > 0) and 100 <= reps[0] and reps[-1] < 100 + n_replicas
    if n_replicas == 64:
        assert np.array_equal(reps, 100 + np.arange(64))           # everything fits: every replica
    else:
        assert len(reps) < n_replicas                             # a sample
    for name, (fid, dt) in LINK_FIELDS.items():
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == dt and np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))   # the same sample every run
        row = t - 1 if name in ("sending_flow", "receiving_flow") else t
        cols = e.n_all if fid < 4 else n_links
        want = e.read_block(fid, row, row + 1)[0][:, (reps - 100).astype(int)].T
        assert a.shape == (len(reps), cols) and np.array_equal(a, want), name


@pytest.mark.gpu
def test_dump_outputs_repeat_and_match_the_oracle(tmp_path):
    """Two runs of the same command dump the same arrays bit for bit, and those are the CPU oracle's rows of the last timed step
    for the same replicas (same Philox keys, same per-replica demand)."""
    import oracle_driver as od
    from golden_util import DATA
    from pednstream_amd import NetworkEnvGenerator
    from pednstream_amd.flatten import flatten_network
    from pednstream_amd.network import LINK_FIELDS

    sys.path.insert(0, ROOT)
    import bench

    steps, warmup, R = 7, 4, 64
    dirs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--network", "nine_intersections", "--replicas", str(R), "--steps", str(steps),
                              "--warmup", str(warmup), "--no-extra", "--no-cpu-baseline", "--no-live-traffic", "--dump-outputs", str(d)],
                             capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        dirs.append(d)
    for name in list(LINK_FIELDS) + ["replicas"]:
        assert np.array_equal(np.load(dirs[0] / (name + ".npy")), np.load(dirs[1] / (name + ".npy"))), name

    net = NetworkEnvGenerator(DATA).create_network("nine_intersections", verbose=False, n_replicas=R, rng_seed=0)
    model, T = flatten_network(net), net.simulation_steps
    t = warmup + steps                          # the clock starts at 1: the last timed step is network_loading(warmup + steps)
    reps = np.load(dirs[0] / "replicas.npy").astype(int)
    assert np.array_equal(reps, np.arange(R))
    for i in (0, R - 1):
        o = od.Oracle(model, seed=0, replica=i)
        for nid in net.origin_nodes:
            o.set_demand(net.nodes[nid].index, bench.replica_demand(T, i))
        o.run(1, t + 1)
        for name in LINK_FIELDS:
            row = t - 1 if name in ("sending_flow", "receiving_flow") else t
            assert np.array_equal(np.load(dirs[0] / (name + ".npy"))[i], o.field(name)[:, row]), (name, i)
        o.close()


@pytest.mark.gpu
def test_plain_run_is_lean():
    """`bench.py --gpus 1 --steps K --warmup W` without --full prints the headline line alone (no roofline, CPU baseline or extras, no
    bench_full.json written) and spends little time outside its steps, set-up included."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    full = os.path.join(ROOT, "bench_full.json")
    before = os.stat(full).st_mtime_ns if os.path.exists(full) else None
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["metric"] == "link-updates/sec (links x replicas x steps/sec)" and d["unit"] == "link-updates/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64+f32" and d["steps"] == steps and d["warmup"] == warmup
    assert abs(d["value"] - 938 * 1024 * steps / (d["ms_per_step"] * steps * 1e-3)) < 1e-3 * d["value"]
    assert not {"roofline", "cpu_baseline", "extra", "full"} & set(d), sorted(d)
    assert (os.stat(full).st_mtime_ns if os.path.exists(full) else None) == before
    assert wall - (steps + warmup) * d["ms_per_step"] * 1e-3 < 30, wall
