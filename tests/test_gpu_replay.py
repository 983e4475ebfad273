"""The replay store on the device (pednstream_amd/replay.py, pednstream_amd/csrc/pedn_replay.hpp) against the contract's numpy
restatement (tests/replay_model.py), fed clones of what the env hands out in the same loop -- bit for bit."""
import numpy as np
import pytest

import replay_model as rp
from golden_util import DATA
from test_gpu_norm import T_SHORT, mixed_env

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0000_0071          # (a key with a high word)
OUT = ("states", "actions", "rewards", "next_states", "dones")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def host(t):
    return t.detach().cpu().numpy()


def policy_of(torch, env, store):
    """Deterministic, and a function of every frame of the stacked observation of ``store()``, the store in use."""
    kept = {}

    def policy(obs):
        st = store().stacked_obs()
        w = torch.arange(1, st.shape[1] + 1, device=st.device, dtype=torch.float64).view(1, -1, 1)
        kept["a"] = ((st[:, :, :env.n_actions].double().abs() * w).sum(1) * 0.7 + 0.5).remainder(3.0).contiguous()
        return kept["a"]
    return policy, kept


def model_of(env, buf):
    return rp.RingModel(buf.capacity, buf.stack_size, T_SHORT, env.n_envs, seed=buf.seed)


def eager_fill(torch, env, buf, model, episodes=3, early=None, awkward=True, check=True):
    """``episodes`` episodes stepped eagerly and pushed, the model fed clones taken in the same loop; ``early``: the second episode
    is cut after that many steps.  ``awkward``: -0.0 and a subnormal go through the actions tensor."""
    policy, _ = policy_of(torch, env, lambda: buf)
    gate = env.action_slices["gate_4"]
    for ep in range(episodes):
        env.reset()
        buf.begin()
        torch.cuda.synchronize()
        model.begin(host(env.device_views()[0].clone()))
        if check:
            assert same(host(buf.stacked_obs()), model.stacked_obs())
        for t in range(early if (early and ep == 1) else T_SHORT):
            a = policy(None)
            if awkward and t in (3, 4):
                a[0, gate.start] = -0.0 if t == 3 else 5e-324
            obs, rew, done = env.step_device(a, sync=t % 2 == 0)
            buf.push(a)
            torch.cuda.synchronize()
            model.push(host(obs.clone()), host(a.clone()), host(rew.clone()), done)
            if check:
                assert same(host(buf.stacked_obs()), model.stacked_obs()), (ep, t)
                assert buf.size_rows() == model.size_rows, (ep, t)
    st = buf.state()
    assert (st["head"], st["steps"], st["size_rows"], st["first"]) == (model.head, model.jhead, model.size_rows, model.cur_first)


def all_sampleable(model):
    return np.array([(s, e) for s in model.sampleable() for e in range(model.N)], dtype=np.int64)


def assert_gathers(torch, env, buf, model, idx, agents=None, out=None):
    """``sample(indices=idx)`` (or the already sampled ``out``) equals the model's gather, for whole rows and for every agent."""
    dev_idx = torch.tensor(idx, device="cuda")
    for aid in ([None] + list(env.possible_agents)) if agents is None else agents:
        if aid is None:
            cols = {}
        else:
            cols = dict(obs=env.obs_slices[aid], act=env.action_slices[aid], rew=env.possible_agents.index(aid))
        want = model.gather(idx, **cols)
        got = out if out is not None else buf.sample(indices=dev_idx, agent=aid)
        torch.cuda.synchronize()
        assert got[5].dtype == torch.int64 and np.array_equal(host(got[5]), idx)
        for name, g, w in zip(OUT, got, want):
            assert same(host(g), w), (aid, name)
        if aid is not None:
            assert got[2].shape == (len(idx),) and got[1].shape == (len(idx), cols["act"].stop - cols["act"].start)


# ---------------------------------------------------------------------------------------------------- eager fills against the model
@pytest.mark.parametrize("capacity,stack,early", [(1, 4, None), (5, 4, None), (5, 1, None), (5, 2, None), (5, 4, 2), (1, 2, 2)])
@pytest.mark.parametrize("n_envs", [1, 3, 65])
def test_eager_fill_equals_the_model(n_envs, capacity, stack, early):
    torch = pytest.importorskip("torch")
    env = mixed_env(n_envs)
    # agent slices that start off a 16-byte boundary, and some that start on one: both copy paths run
    starts = {env.obs_slices[a].start % 4 for a in env.possible_agents}
    assert 0 in starts and len(starts) > 1, starts
    buf = env.replay_store(capacity, stack_size=stack, seed=SEED)
    assert buf.ring_slots == capacity + stack + 1 + 1 and buf.stacked_obs().shape == (n_envs, stack, env.n_obs)
    model = model_of(env, buf)
    eager_fill(torch, env, buf, model, early=early)
    assert model.head > 2 * model.R                              # the ring has wrapped, across episode boundaries
    assert buf.size() == model.size_rows * n_envs > 0
    assert_gathers(torch, env, buf, model, all_sampleable(model))
    assert buf.nbytes >= sum(v.numel() * v.element_size() for v in buf.views().values())
    buf.close()
    env.close()


def test_awkward_values_come_back_bit_for_bit():
    torch = pytest.importorskip("torch")
    env = mixed_env(3)
    buf = env.replay_store(T_SHORT, stack_size=4, seed=SEED)
    model = model_of(env, buf)
    eager_fill(torch, env, buf, model, episodes=1, check=False)
    # a NaN with a payload, -0.0 and a subnormal straight into the ring's frames and rewards, and into the model's
    v = buf.views()
    s = model.sampleable()[5]
    slot = s % model.R
    odd = torch.from_numpy(np.array([0x7FC12345, 0x80000000, 0x00000001], dtype=np.uint32).view(np.float32)).cuda()
    v["frames"][slot, 1, 1:4] = odd
    v["rewards"][slot, 2, :3] = odd
    model.frames[slot][1, 1:4] = host(odd)
    model.rewards[slot][2, :3] = host(odd)
    idx = all_sampleable(model)
    assert_gathers(torch, env, buf, model, idx)
    got = buf.sample(indices=torch.tensor(idx, device="cuda"))
    assert (bits(host(got[0])) == 0x7FC12345).any() and (bits(host(got[1])) == 1).any() and (bits(host(got[1])) == 1 << 63).any()
    # (and the episode is not a trivial one: frames move, rewards are paid, the last row is the terminated one)
    assert not same(host(got[0]), host(got[3])) and (host(got[2]) != 0).any() and host(got[4]).sum() == 3 and host(got[4])[-3:].all()
    env.close()


# ---------------------------------------------------------------------------------------------------- random minibatches
@pytest.mark.parametrize("n_envs", [3, 65])
def test_random_samples_are_the_models_draws(n_envs):
    torch = pytest.importorskip("torch")
    env = mixed_env(n_envs)
    buf = env.replay_store(5, stack_size=4, seed=SEED)
    model = model_of(env, buf)
    eager_fill(torch, env, buf, model, episodes=2, early=7, check=False)
    agents = [None] + list(env.possible_agents)
    for n, B in enumerate((1, 63, 64, 257, 64)):
        aid = agents[n % len(agents)]
        idx = model.draw(B)
        out = buf.sample(B, agent=aid)
        assert_gathers(torch, env, buf, model, idx, agents=[aid], out=out)
        # every agent's columns of the same draw; the draw counter stays
        assert_gathers(torch, env, buf, model, idx, agents=[a for a in agents if a != aid][:1])
    first = buf.sample(64, agent=agents[0])
    again = buf.sample(64, agent=agents[0])
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(first, again))          # allocated once, reused
    model.draws += 2
    assert buf.state()["draws"] == model.draws == 7
    env.close()


def test_a_captured_sample_draws_anew_at_every_replay():
    torch = pytest.importorskip("torch")
    env = mixed_env(3)
    buf = env.replay_store(5, stack_size=2, seed=SEED)
    model = model_of(env, buf)
    eager_fill(torch, env, buf, model, episodes=1, check=False)
    aid = "gate_4"
    out = buf.sample(64, agent=aid)                    # (allocates the outputs; draw 0)
    model.draw(64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):             # one stream, one launch
        captured = buf.sample(64, agent=aid)
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(out, captured))
    for d in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        assert model.draws == d
        assert_gathers(torch, env, buf, model, model.draw(64), agents=[aid], out=captured)
    assert buf.state()["draws"] == 3
    env.close()


# ---------------------------------------------------------------------------------------------------- captured rollouts
def ring_image(buf):
    st = buf.state()
    return {**{k: host(v) for k, v in buf.views().items()}, "state": np.array([st[k] for k in ("head", "steps", "size_rows", "first")])}


def captured_fill(torch, env, buf, n, episodes=2):
    policy, kept = policy_of(torch, env, lambda: buf)
    roll = env.capture(policy, on_step=lambda obs, rew: buf.push(kept["a"]), steps_per_replay=n)
    for _ in range(episodes):
        env.reset()
        buf.begin()
        while not roll.step():
            pass
    return roll


@pytest.mark.parametrize("n_envs", [3, 65])
def test_a_captured_rollout_fills_the_ring_with_the_same_bits(n_envs):
    torch = pytest.importorskip("torch")
    env = mixed_env(n_envs)
    buf = env.replay_store(T_SHORT + 3, stack_size=4, seed=SEED)
    model = model_of(env, buf)
    eager_fill(torch, env, buf, model, episodes=2, awkward=False, check=False)
    want = ring_image(buf)
    assert want["done"].sum() == 2 and want["state"][0] == 2 * T_SHORT + 2
    env.close()
    for n in (1, 3):
        env = mixed_env(n_envs)
        buf = env.replay_store(T_SHORT + 3, stack_size=4, seed=SEED)
        roll = captured_fill(torch, env, buf, n)
        assert roll.replays > 0 and roll.recaptures == 0
        got = ring_image(buf)
        for k in want:
            assert same(got[k], want[k]), (n, k)
        assert_gathers(torch, env, buf, model, all_sampleable(model)[::7], agents=[None, "gate_4"])
        env.close()


def test_store_holds_the_normalised_rows_while_the_running_normalisation_is_on():
    torch = pytest.importorskip("torch")
    env = mixed_env(65)
    env.set_running_norm(norm_obs=True, norm_reward=True)
    buf = env.replay_store(5, stack_size=4, seed=SEED)
    model = model_of(env, buf)
    eager_fill(torch, env, buf, model, episodes=1)          # (the model is fed device_views(): the normalised rows)
    torch.cuda.synchronize()
    newest = (model.head - 1) % model.R
    v = buf.views()
    assert same(host(v["frames"][newest]), host(env.device_views()[0])) and not same(host(v["frames"][newest]), host(env.raw_views()[0]))
    assert same(host(v["rewards"][newest]), host(env.device_views()[1])) and not same(host(v["rewards"][newest]), host(env.raw_views()[1]))
    assert_gathers(torch, env, buf, model, all_sampleable(model)[::5])
    env.close()


# ---------------------------------------------------------------------------------------------------- refusals, the error flag
def test_refusals():
    torch = pytest.importorskip("torch")
    from pednstream_amd.rl_env import MultiScenarioVecEnv

    multi = MultiScenarioVecEnv("long_corridor", n_envs=2, group_size=1, data_dir=DATA)
    with pytest.raises(ValueError):
        multi.replay_store(4)
    multi.close()
    env = mixed_env(3)
    for bad in (dict(capacity=0), dict(capacity=4, stack_size=0)):
        with pytest.raises(ValueError):
            env.replay_store(**bad)
    buf = env.replay_store(4, stack_size=2)
    a = torch.zeros(3, env.n_actions, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        buf.push(a)                                              # before begin()
    env.reset()
    buf.begin()
    for bad in (a.float(), a[:2], a.cpu(), a.t().contiguous().t(), a[:, :-1]):
        with pytest.raises(ValueError):
            buf.push(bad)
    with pytest.raises(ValueError):
        buf.sample(4)                                            # the host knows nothing has been pushed
    env.step_device(a)
    buf.push(a)
    ok = torch.tensor([[1, 0]], device="cuda")
    for bad in (dict(batch_size=0), dict(batch_size=None), dict(indices=ok.int()), dict(indices=ok[0]), dict(indices=ok.cpu()),
                dict(indices=ok.expand(2, 2).t()), dict(indices=ok, batch_size=2), dict(batch_size=2, agent="nobody")):
        with pytest.raises(ValueError):
            buf.sample(**bad)
    assert buf.sample(indices=ok)[0].shape == (1, 2, env.n_obs) and buf.size() == 3
    env.close()


def test_an_index_that_is_not_sampleable_raises_the_flag_and_writes_nothing():
    torch = pytest.importorskip("torch")
    env = mixed_env(3)
    buf = env.replay_store(2, stack_size=2, seed=SEED)
    model = model_of(env, buf)
    eager_fill(torch, env, buf, model, episodes=2, early=1, check=False)
    good = model.sampleable()                                # the last row of the first episode and the one row of the second
    reset_row = model.cur_first                              # between them, inside the ring
    assert good == [reset_row - 1, reset_row + 1] and model.first[reset_row % model.R] == -1 and reset_row >= model.head - model.R
    assert model.first[(good[0] - 1) % model.R] >= 0         # a STEP row inside the ring that has left the newest `capacity`
    bad = [(good[0] - 1, 0), (reset_row, 1), (model.head, 0), (model.head + 10 ** 12, 0), (-1, 0), (good[-1], 3), (good[-1], -1),
           (good[0] - model.R, 0), (-2 ** 62, 0)]
    idx = torch.tensor(bad + [(good[-1], 2)], device="cuda")
    out = buf.sample(indices=idx)
    for t in out[:5]:
        t.fill_(7.0)
    buf.sample(indices=idx)
    torch.cuda.synchronize()
    for name, t, w in zip(OUT, out, model.gather([(good[-1], 2)])):
        assert (host(t[:-1]) == 7.0).all(), name             # untouched rows
        assert same(host(t[-1:]), w), name                   # the one good index beside them is served
    with pytest.raises(RuntimeError):
        buf.size()
    assert buf.size() == 2 * 3                               # reported once
    # a store the device knows to be empty: the only STEP row is pushed out of the ring by RESET rows
    buf = env.replay_store(1, stack_size=1, seed=SEED)
    model = model_of(env, buf)
    eager_fill(torch, env, buf, model, episodes=1, check=False)
    out = buf.sample(5)
    model.draws += 1
    for _ in range(model.R):
        buf.begin()
        model.begin(host(env.device_views()[0]))
    assert model.size_rows == 0
    for t in out[:5]:
        t.fill_(7.0)
    buf.sample(5)
    torch.cuda.synchronize()
    assert all((host(t) == 7.0).all() for t in out[:5])
    with pytest.raises(RuntimeError):
        buf.close()
    env.close()


# ---------------------------------------------------------------------------------------------------- beside a rollout store
def test_a_rollout_store_and_a_replay_store_live_side_by_side():
    torch = pytest.importorskip("torch")
    from test_gpu_rollout import same as same32

    n_envs = 3
    env = mixed_env(n_envs)
    store = env.rollout_store()
    buf = env.replay_store(7, stack_size=4, seed=SEED)
    model = model_of(env, buf)
    policy, kept = policy_of(torch, env, lambda: buf)
    log = {"actions": [], "rewards": [], "obs": []}

    def on_step(obs, rew):
        store.record(kept["a"])
        buf.push(kept["a"])
    roll = env.capture(policy, on_step=on_step)

    def episode(keep):
        env.reset()
        store.begin()
        buf.begin()
        torch.cuda.synchronize()
        model.begin(host(env.device_views()[0]))
        if keep:
            log["obs"].append(host(env.device_views()[0]))
        done = False
        while not done:
            done = roll.step()
            torch.cuda.synchronize()
            obs, rew = env.device_views()
            model.push(host(obs), host(kept["a"]), host(rew), done)
            if keep:
                for k, t in (("actions", kept["a"]), ("rewards", rew), ("obs", obs)):
                    log[k].append(host(t))
    episode(True)
    assert roll.recaptures == 0 and store.finish() == T_SHORT
    views = store.views()
    for k in log:
        assert same32(host(views[k]), np.stack(log[k])), k
    assert buf.size_rows() == model.size_rows == 7
    assert_gathers(torch, env, buf, model, all_sampleable(model), agents=[None, "sep_0" if "sep_0" in env.possible_agents else env.possible_agents[0]])
    # reconfiguring either store makes the captured rollout capture again
    buf = env.replay_store(7, stack_size=2, seed=SEED)
    model = model_of(env, buf)
    episode(False)
    assert roll.recaptures == 1
    assert_gathers(torch, env, buf, model, all_sampleable(model), agents=[None])
    store = env.rollout_store(capacity=T_SHORT + 1)
    episode(False)
    assert roll.recaptures == 2 and store.finish() == T_SHORT
    assert_gathers(torch, env, buf, model, all_sampleable(model), agents=[None])
    env.close()
