"""The rollout store and the advantage kernels on the device (pednstream_amd/rollout.py, pednstream_amd/csrc/pedn_rollout.hpp) against the
contract's numpy restatement (tests/rollout_model.py), the reference's own compute_gae (goldens gae_*.npz) and plain torch clones taken
in an eager loop -- bit for bit."""
import functools

import numpy as np
import pytest

import rollout_model as rm
from pednstream_amd import rollout
from pednstream_amd.rl_env import _DeviceBuffer
from test_gpu_controllers import device_agents, make_env
from test_gpu_norm import T_SHORT, mixed_env
from test_rollout_contract import GAE_CASES, load_gae

pytestmark = pytest.mark.gpu

UNROLL = 8          # PEDN_GAE_UNROLL: rows per block of the GAE kernel
GAMMA, LMBDA = 0.99, 0.95
assert float(np.float32(GAMMA * LMBDA)) != GAMMA * LMBDA


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def awkward(rng, shape, scale):
    """Normal values with +-0.0 and subnormals mixed in."""
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    kind = rng.integers(0, 10, size=shape)
    x[kind == 0] = 0.0
    x[kind == 1] = -0.0
    tiny = (rng.integers(1, 1 << 22, size=shape).astype(np.uint32) | (rng.integers(0, 2, size=shape).astype(np.uint32) << 31)).view(np.float32)
    x[kind == 2] = tiny[kind == 2]
    return x


# ---------------------------------------------------------------------------------------------------- gae() on synthetic tensors
@pytest.mark.parametrize("T", [1, 2, UNROLL - 1, UNROLL, UNROLL + 1, 2 * UNROLL, 64, 65])
def test_gae_equals_the_model(T):
    torch = pytest.importorskip("torch")
    for lanes in (1, 63, 64, 65, 257, 1000):
        rng = np.random.default_rng(1000 * T + lanes)
        r, v = awkward(rng, (T, lanes), 3.0), awkward(rng, (T + 1, lanes), 20.0)
        d = (rng.integers(0, 5, size=(T, lanes)) == 0).astype(np.float32)
        assert lanes < 64 or ((bits(v) == 0x80000000).any() and (np.abs(v[v != 0]) < np.finfo(np.float32).tiny).any())
        td0, adv0 = rm.td_and_gae(r, v, d, GAMMA, LMBDA)
        adv, td = rollout.gae(torch.tensor(r).cuda(), torch.tensor(v).cuda(), torch.tensor(d).cuda(), GAMMA, LMBDA)
        assert same(td.cpu().numpy(), td0), (T, lanes)
        assert same(adv.cpu().numpy(), adv0), (T, lanes)
    # trailing axes are flattened: [T, 5, 200] is the 1000-lane case
    adv3, td3 = rollout.gae(torch.tensor(r).cuda().view(T, 5, 200), torch.tensor(v).cuda().view(T + 1, 5, 200), torch.tensor(d).cuda().view(T, 5, 200),
                            GAMMA, LMBDA)
    assert adv3.shape == (T, 5, 200) and same(adv3.cpu().numpy().reshape(T, 1000), adv0) and same(td3.cpu().numpy().reshape(T, 1000), td0)


@pytest.mark.parametrize("case", GAE_CASES)
def test_gae_reproduces_the_reference_bits(case):
    torch = pytest.importorskip("torch")
    z, _ = load_gae(case)
    g, l = float(z["gamma"]), float(z["lmbda"])
    adv, td = rollout.gae(torch.tensor(z["rewards"]).cuda(), torch.tensor(z["values"]).cuda(), torch.tensor(z["dones"]).cuda(), g, l)
    assert same(td.cpu().numpy(), z["td_target"]) and same(adv.cpu().numpy(), z["adv"])
    # the reference's own signature: td_delta (T, 1) or (T,), CPU or CUDA, same shape and device back
    delta = torch.tensor(z["td_target"] - z["values"][:-1])
    for x in (delta.view(-1, 1), delta, delta.view(-1, 1).cuda()):
        out = rollout.compute_gae(g, l, x)
        assert out.dtype == torch.float32 and out.shape == x.shape and out.device == x.device
        assert same(out.cpu().numpy().reshape(-1), z["adv"])


def test_gae_refusals():
    torch = pytest.importorskip("torch")
    r, v = torch.zeros(4, 3, device="cuda"), torch.zeros(5, 3, device="cuda")
    for bad in ((r.double(), v, r), (r, v[:4], r), (r, v, r[:3]), (r, v.cpu(), r), (r[:0], v[:1], r[:0])):
        with pytest.raises(ValueError):
            rollout.gae(*bad, GAMMA, LMBDA)


# ---------------------------------------------------------------------------------------------------- the store on a small env
def heads(torch, env):
    """A policy and a critic that depend on the observation they are handed; the critic's output is V of the state the action is
    decided in, so both are evaluated before the step and kept for ``record``."""
    n_agents = len(env.possible_agents)
    kept = {}

    def policy(obs):
        kept["a"] = (obs[:, :env.n_actions].double().abs() * 0.7 + 0.5).remainder(3.0).contiguous()
        kept["v"] = (obs[:, -n_agents:] * 0.25 - obs[:, :n_agents] + 1.5).contiguous()
        return kept["a"]
    return policy, kept


def fill(torch, env, how, store=None, steps=None, norm=None):
    """One episode (or ``steps`` policy steps of one) stepped ``how``; with a store: recorded into it, without: torch clones of what a
    store has to hold, as numpy arrays."""
    if norm:
        env.set_running_norm(**norm)
    policy, kept = heads(torch, env)
    log = {k: [] for k in ("actions", "values", "rewards", "done", "obs")}
    roll = None
    if how.startswith("graph"):
        roll = env.capture(policy, on_step=lambda obs, rew: store.record(kept["a"], kept["v"]), steps_per_replay=int(how[-1]))
    env.reset()
    if store is not None:
        store.begin()
    else:
        torch.cuda.synchronize()
        log["obs"].append(env.device_views()[0].clone())
    done, n = False, 0
    while not done and (steps is None or n < steps):
        if roll is not None:
            done = roll.step()               # (whole episodes only)
            continue
        a = policy(env.device_views()[0])
        o, r, done = env.step_device(a, sync=how == "device_sync")
        n += 1
        if store is not None:
            store.record(a, kept["v"])
        else:
            torch.cuda.synchronize()
            for k, t in (("actions", a), ("values", kept["v"]), ("rewards", r), ("obs", o)):
                log[k].append(t.clone())
            log["done"].append(torch.full((env.n_envs,), float(done), device="cuda"))
    if store is not None:
        return roll
    torch.cuda.synchronize()
    return {k: torch.stack(v).cpu().numpy() for k, v in log.items()}


@functools.lru_cache(maxsize=None)
def eager_reference(n_envs, norm=False):
    """What a store must hold after a whole episode of mixed_env: computed once per batch size, shared, never changed."""
    import torch

    env = mixed_env(n_envs)
    ref = fill(torch, env, "device_sync", norm=NORM if norm else None)
    env.close()
    for v in ref.values():
        v.setflags(write=False)
    assert ref["rewards"].shape == (T_SHORT, n_envs, 3) and ref["obs"].shape[0] == T_SHORT + 1
    return ref


NORM = dict(norm_obs=True, norm_reward=True, gamma=0.9)


def fetched(store):
    return {k: v.cpu().numpy() for k, v in store.views().items()}


def assert_holds(store, ref, rows=T_SHORT, first=0):
    got = fetched(store)
    for k in ("actions", "values", "rewards", "done", "obs"):
        want = ref[k][first:first + rows + (1 if k == "obs" else 0)]
        have = got[k][:rows] if k == "values" else got[k]
        assert same(have, want), k
    return got


@pytest.mark.parametrize("n_envs", [1, 3, 65, 130])
def test_every_way_of_stepping_fills_the_store_with_the_same_bits(n_envs):
    torch = pytest.importorskip("torch")
    ref = eager_reference(n_envs)
    assert ref["done"][:-1].sum() == 0 and (ref["done"][-1] == 1).all()          # 1 on the terminated row only
    assert (ref["rewards"] != 0).any() and not same(ref["obs"][0], ref["obs"][-1])
    for how in ("device_sync", "device_async", "graph1", "graph3"):
        env = mixed_env(n_envs)
        store = env.rollout_store()
        assert store.capacity == T_SHORT
        roll = fill(torch, env, how, store)
        assert store.finish() == T_SHORT and not store.overflow, how
        if roll is not None:
            assert roll.replays == {"graph1": T_SHORT - 1, "graph3": (T_SHORT - 1) // 3}[how] and roll.recaptures == 0
            assert roll.eager_steps == T_SHORT - roll.replays * roll.n
        got = assert_holds(store, ref)
        assert same(got["obs"][0], ref["obs"][0])                                 # the reset observation
        assert got["values"].shape == (T_SHORT + 1, n_envs, 3) and not got["values"][-1].any()          # the default bootstrap row
        one = store.agent("gate_4")
        assert one["obs"].shape[-1] == env.obs_slices["gate_4"].stop - env.obs_slices["gate_4"].start
        assert torch.equal(one["rewards"], store.views()["rewards"][..., env.possible_agents.index("gate_4")])
        assert one["actions"].data_ptr() == store.views()["actions"][..., env.action_slices["gate_4"]].data_ptr()     # views, not copies
        env.close()


def test_store_holds_the_normalised_rows_while_the_running_normalisation_is_on():
    torch = pytest.importorskip("torch")
    n_envs = 65
    ref, raw = eager_reference(n_envs, True), eager_reference(n_envs)
    assert not same(ref["obs"], raw["obs"]) and not same(ref["rewards"], raw["rewards"])
    for how in ("device_async", "graph3"):
        env = mixed_env(n_envs)
        env.set_running_norm(**NORM)              # before the store ...
        store = env.rollout_store()
        fill(torch, env, how, store)
        assert store.finish() == T_SHORT
        assert_holds(store, ref)
        env.close()
    env = mixed_env(n_envs)                       # ... or after it: the store follows the buffers the env hands out
    store = env.rollout_store()
    fill(torch, env, "graph1", store, norm=NORM)
    assert store.finish() == T_SHORT
    assert_holds(store, ref)
    env.close()


def test_store_with_controllers():
    torch = pytest.importorskip("torch")
    n_envs, steps = 3, 12
    logs = []
    for with_store in (False, True):
        g, info, env = make_env("ctrl_one_gate3", n_envs)
        env.set_controllers(device_agents(env, info))
        eng = env.network.engine()
        rows = torch.as_tensor(_DeviceBuffer(eng.ctrl_device_ptr(0), (n_envs, env.n_actions), "<f8"), device="cuda")
        store = env.rollout_store(capacity=steps) if with_store else None
        env.reset()
        log = {k: [] for k in ("actions", "rewards", "obs")}
        if store is not None:
            store.begin()
        else:
            log["obs"].append(env.device_views()[0].clone())
        for _ in range(steps):
            eng.synchronize()
            a = rows.clone()                      # the controllers' action rows: what the step about to run applies
            env.step_controlled(1, fetch=False)
            if store is not None:
                store.record(a)
            else:
                eng.synchronize()
                log["actions"].append(a)
                log["rewards"].append(env.device_views()[1].clone())
                log["obs"].append(env.device_views()[0].clone())
        if store is not None:
            assert store.finish() == steps
            logs.append(fetched(store))
        else:
            logs.append({k: torch.stack(v).cpu().numpy() for k, v in log.items()})
        env.close()
    want, got = logs
    assert np.isfinite(want["actions"]).any() and (want["rewards"] != 0).any()
    for k in ("actions", "rewards", "obs"):
        assert want[k].tobytes() == got[k].tobytes(), k
    assert not got["values"].any() and not got["done"].any()


# ---------------------------------------------------------------------------------------------------- compute_gae on a filled store
def test_compute_gae_on_a_filled_store_equals_the_model():
    torch = pytest.importorskip("torch")
    n_envs = 65
    env = mixed_env(n_envs)
    store = env.rollout_store()
    with pytest.raises(ValueError):
        store.record(torch.zeros(n_envs, env.n_actions, dtype=torch.float64, device="cuda"))        # before begin()
    fill(torch, env, "graph3", store)
    with pytest.raises(ValueError):
        store.compute_gae(GAMMA, LMBDA)                                                              # before finish()
    last = torch.tensor(awkward(np.random.default_rng(2), (n_envs, 3), 5.0)).cuda()
    for bad in (last.double(), last[:, :2], last.cpu()):
        with pytest.raises(ValueError):
            store.finish(bad)
    assert store.finish(last) == T_SHORT
    got = assert_holds(store, eager_reference(n_envs))
    assert same(got["values"][-1], last.cpu().numpy())
    done3 = np.broadcast_to(got["done"][:, :, None], got["rewards"].shape)
    td0, adv0 = rm.td_and_gae(got["rewards"], got["values"], done3, GAMMA, LMBDA)
    adv, td = store.compute_gae(GAMMA, LMBDA)
    assert adv.shape == (T_SHORT, n_envs, 3) and adv.data_ptr() == store.views()["advantages_raw"].data_ptr()
    assert same(td.cpu().numpy(), td0) and same(adv.cpu().numpy(), adv0)
    adv_n, td = store.compute_gae(GAMMA, LMBDA, normalize=True)
    assert same(td.cpu().numpy(), td0) and same(store.views()["advantages_raw"].cpu().numpy(), adv0)
    assert same(adv_n.cpu().numpy(), rm.normalize_advantages(adv0))
    assert abs(float(adv_n[..., 1].double().mean())) < 1e-6 and abs(float(adv_n[..., 1].double().std()) - 1.0) < 1e-5
    # the functional form on the same arrays
    adv_f, td_f = rollout.gae(store.views()["rewards"], store.views()["values"], store.views()["done"][:, :, None].expand(-1, -1, 3), GAMMA, LMBDA)
    assert same(adv_f.cpu().numpy(), adv0) and same(td_f.cpu().numpy(), td0)
    # agents are independent: another agent's rewards permuted (over rows and envs) leave this agent's numbers alone
    keep_n = adv_n.cpu().numpy().copy()
    rew = store.views()["rewards"]
    col = rew[:, :, 2].reshape(-1)
    rew[:, :, 2] = col[torch.randperm(col.numel(), device="cuda")].view(T_SHORT, n_envs)
    adv_n2, _ = store.compute_gae(GAMMA, LMBDA, normalize=True)
    now = adv_n2.cpu().numpy()
    assert same(now[..., :2], keep_n[..., :2]) and not same(now[..., 2], keep_n[..., 2])
    env.close()


def test_normalisation_needs_two_entries():
    torch = pytest.importorskip("torch")
    env = mixed_env(1)
    store = env.rollout_store(capacity=2, store_obs=False)
    assert "obs" not in store.views()
    fill(torch, env, "device_sync", store, steps=1)
    assert store.finish() == 1
    store.compute_gae(GAMMA, LMBDA)
    with pytest.raises(ValueError):
        store.compute_gae(GAMMA, LMBDA, normalize=True)
    with pytest.raises(ValueError):
        env.network.engine().rollout_compute(GAMMA, LMBDA, True)          # the C entry point refuses too
    env.close()


# ---------------------------------------------------------------------------------------------------- overflow, a second fill, re-capture
def test_overflow_keeps_the_prefix_and_begin_starts_a_clean_fill():
    torch = pytest.importorskip("torch")
    n_envs, cap = 3, 10
    ref = eager_reference(n_envs)
    env = mixed_env(n_envs)
    store = env.rollout_store(capacity=cap)
    fill(torch, env, "graph1", store)
    assert store.finish() == cap and store.overflow
    assert_holds(store, ref, rows=cap)
    fill(torch, env, "device_async", store, steps=5)          # reset() + begin(): the same episode again, five rows of it
    assert store.finish() == 5 and not store.overflow
    assert_holds(store, ref, rows=5)
    adv, td = store.compute_gae(GAMMA, LMBDA)
    assert adv.shape == (5, n_envs, 3)
    env.close()


def test_a_store_configured_after_a_capture_is_captured_again():
    torch = pytest.importorskip("torch")
    n_envs, before = 65, 7
    ref = eager_reference(n_envs)
    env = mixed_env(n_envs)
    policy, kept = heads(torch, env)
    box = {"store": None}

    def on_step(obs, rew):
        if box["store"] is not None:
            box["store"].record(kept["a"], kept["v"])
    roll = env.capture(policy, on_step=on_step)
    env.reset()
    for _ in range(before):
        roll.step()
    assert roll.replays == before - 1 and roll.recaptures == 0
    box["store"] = store = env.rollout_store()
    store.begin()                                                 # a fill may start inside an episode: row 0 is the next step
    done = False
    while not done:
        done = roll.step()
    assert roll.recaptures == 1
    rows = T_SHORT - before
    assert store.finish() == rows and not store.overflow
    assert_holds(store, ref, rows=rows, first=before)
    env.close()
