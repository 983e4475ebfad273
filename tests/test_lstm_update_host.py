"""Host side of the recurrent agents' clipped-loss epochs (pednstream_amd/lstm.py: LstmPpoTargets.epoch_update, epoch_gradients,
update_store, begin_update): the entry points, the workspace's size and every refusal that needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from pednstream_amd import engine, lstm, ppo
from pednstream_amd.rollout import RolloutStore

AGENTS = [(0, 1, 0, 1), (2, 33, 1, 8), (36, 20, 9, 3)]       # (obs0, obs_w, act0, act_w) with gaps between their columns (section 17's)
N_OBS, N_ACT = 57, 12


def make(n_envs=1):
    actors = lstm.LstmActors(AGENTS, low=np.zeros(N_ACT), high=np.full(N_ACT, 4.0), n_envs=n_envs, n_obs=N_OBS, n_actions=N_ACT, delta_actions=False)
    return lstm.LstmPpoTargets(actors)


def test_the_entry_points_are_declared_at_the_end_of_the_header():
    assert engine.ABI_VERSION == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pedn.h")).read()
    a, b = header.index("int pedn_lstm_ppo_epoch_update(const float* obs"), header.index("int pedn_lstm_ppo_begin_update(int32_t* stop_flags")
    assert header.index("int pedn_device_math(") < a < b and "int pedn_" not in header[b + 10:]
    assert "pedn_lstm_ppo_epoch_update" in engine.EXPORTS and "pedn_lstm_ppo_begin_update" in engine.EXPORTS
    lib = engine.lib()
    assert lib.pedn_lstm_ppo_epoch_update and lib.pedn_lstm_ppo_begin_update


def test_the_interface_mirrors_the_stacked_agents():
    import inspect

    for name in ("epoch_update", "epoch_gradients", "update_store"):
        mine, theirs = (inspect.signature(getattr(c, name)) for c in (lstm.LstmPpoTargets, ppo.PpoTargets))
        assert list(mine.parameters) == list(theirs.parameters), name
        assert [p.default for p in mine.parameters.values()] == [p.default for p in theirs.parameters.values()], name
    for name in ("begin_update", "epoch_outputs", "adam_state", "adam_steps", "reset_adam"):
        assert hasattr(lstm.LstmPpoTargets, name)


def test_workspace_bytes_follow_the_formula():
    t = make()
    lstm_floats = lambda ow: 256 * (ow + 64 + 2)
    apack = t.actors.pack_size
    assert apack == sum(-(-(lstm_floats(ow) + 2 * (64 * aw + aw)) // 4) * 4 for (_, ow, _, aw) in AGENTS)
    vpack = t.pack_size
    assert vpack == sum(-(-(lstm_floats(ow) + 65) // 4) * 4 for (_, ow, _, _) in AGENTS)
    slab = -(-apack // 4) * 4 + vpack + 8 * 3
    for (T, N, g) in ((1, 1, 1), (1, 32, 3), (3, 11, 3), (97, 1, 2), (97, 1, 64), (700, 2048, None)):
        R = T * N
        G = min(-(-R // 32), ppo.DEFAULT_GROUPS if g is None else g)
        assert t.update_workspace_bytes(T, N, g) == 4 * (2 * 3 * R * 384 + 4 * R * N_ACT + G * slab), (T, N, g)
    assert lstm.ROW_FLOATS == 384 and lstm.TAIL_PLANES == 4
    # the activations dominate: about 2.2 GB per network and agent at 700 x 2048 rows
    assert 2.1e9 < 700 * 2048 * 384 * 4 < 2.3e9
    for bad in ((0, 4), (4, 0), (1.5, 4), (True, 4)):
        with pytest.raises(ValueError, match="T and N"):
            t.update_workspace_bytes(*bad)
    with pytest.raises(ValueError, match="groups"):
        t.update_workspace_bytes(4, 4, 0)


def fake_store(t, **kw):
    s = RolloutStore.__new__(RolloutStore)
    s.store_obs, s.rows, s.n_obs, s.n_actions, s.n_agents = True, 3, t.n_obs, t.n_actions, t.n_agents
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_refusals_that_need_no_device():
    torch = pytest.importorskip("torch")
    t = make()
    T, N = 3, 2
    obs, act, old = torch.zeros(T + 1, N, N_OBS), torch.zeros(T, N, N_ACT), torch.zeros(T, N, N_ACT)
    adv, td = torch.zeros(T, N, 3), torch.zeros(T, N, 3)
    args = (obs, act, old, adv, td)
    for bad in (float("nan"), float("inf"), -1e-3, "x", None):
        with pytest.raises(ValueError, match="actor_lr|numbers"):
            t.epoch_update(*args, actor_lr=bad)
        with pytest.raises(ValueError, match="critic_lr|numbers"):
            t.epoch_update(*args, critic_lr=bad)
    for bad in (float("nan"), float("inf"), -1e-8):
        with pytest.raises(ValueError, match="eps"):
            t.epoch_update(*args, eps=bad)
    for bad in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, float("nan")), (0.9,), (0.9, 0.99, 0.999), 0.9):
        with pytest.raises(ValueError, match="betas"):
            t.epoch_update(*args, betas=bad)
    for bad in (float("nan"), float("inf"), 0.0, -0.2):
        with pytest.raises(ValueError, match="clip_eps"):
            t.epoch_update(*args, clip_eps=bad)
        with pytest.raises(ValueError, match="clip_eps"):
            t.epoch_gradients(*args, clip_eps=bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            t.epoch_update(*args, max_grad_norm=bad)
    with pytest.raises(ValueError, match="kl_tolerance"):
        t.epoch_update(*args, kl_tolerance=float("nan"))
    for bad in (0, -1, 1.5, True, 65536, "2"):
        with pytest.raises(ValueError, match="groups"):
            t.epoch_update(*args, groups=bad)
    # shapes, dtypes, devices, contiguity: the first thing wrong is named
    for bad in (None, np.zeros((T + 1, N, N_OBS), dtype=np.float32), torch.zeros(N, N_OBS), torch.zeros(1, N, N_OBS)):
        with pytest.raises(ValueError, match="obs must"):
            t.epoch_update(bad, act, old, adv, td)
    with pytest.raises(ValueError, match="obs must be on cuda"):
        t.epoch_update(*args)                                   # CPU tensors
    with pytest.raises(ValueError, match="obs must be on cuda"):
        t.epoch_gradients(*args)
    with pytest.raises(ValueError, match="obs must"):
        t.epoch_update(torch.zeros(T + 1, N, N_OBS + 1), act, old, adv, td)
    with pytest.raises(ValueError, match="obs must"):
        t.epoch_update(torch.zeros(T + 1, N, N_OBS, dtype=torch.float64), act, old, adv, td)
    with pytest.raises(ValueError, match="obs must"):
        t.epoch_update(torch.zeros(T + 1, N_OBS, N).transpose(1, 2), act, old, adv, td)
    # update_store: epochs, groups, and what the store must be
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="epochs"):
            t.update_store(fake_store(t), old, adv, td, epochs=bad)
    with pytest.raises(ValueError, match="groups"):
        t.update_store(fake_store(t), old, adv, td, groups=0)
    with pytest.raises(ValueError, match="RolloutStore"):
        t.update_store(object(), old, adv, td)
    with pytest.raises(ValueError, match="keeps no observations"):
        t.update_store(fake_store(t, store_obs=False), old, adv, td)
    with pytest.raises(ValueError, match="finish"):
        t.update_store(fake_store(t, rows=None), old, adv, td)
    with pytest.raises(ValueError, match="no rows"):
        t.update_store(fake_store(t, rows=0), old, adv, td)
    with pytest.raises(ValueError, match="not made for the env"):
        t.update_store(fake_store(t, n_obs=N_OBS - 1), old, adv, td)
    with pytest.raises(ValueError, match="epoch_update\\(\\) has not run"):
        t.epoch_outputs
    with pytest.raises(ValueError, match="Unknown agent"):
        t.adam_state(7, "actor")
    with pytest.raises(ValueError, match="which must be"):
        t.adam_state(0, "critic")
    # unloaded networks (the check every epoch call makes behind its tensors')
    with pytest.raises(ValueError, match="no parameters were loaded"):
        t._check_loaded()
    t.actors._loaded.update(range(3))
    with pytest.raises(ValueError, match="no value networks were loaded"):
        t._check_loaded()
    assert t._udev is None and t._dev is None and t.actors._dev is None      # nothing above touched a device


def test_refusals_at_the_c_abi():
    lib = engine.lib()
    ok = [C.c_void_p(4096 + 256 * i) for i in range(26)]      # never read: every call below is refused before a launch
    tail = [10000, 8000, 3, 2, N_OBS, N_ACT, 3, 64, 1, 0, 4, 1e-3, 10.0, 3e-4, 6e-4, 0.2, 0.5, 0.01, 0.9, 0.999, 1e-8, 1, None]

    def call(ptrs=None, **kw):
        names = ["apack", "vpack", "T", "N", "n_obs", "n_actions", "n_agents", "hidden", "layers", "f64", "groups", "min_std", "max_std", "actor_lr",
                 "critic_lr", "clip_eps", "max_grad_norm", "kl_tolerance", "beta1", "beta2", "eps", "do_adam", "stream"]
        vals = list(tail)
        for k, v in kw.items():
            vals[names.index(k)] = v
        rc = lib.pedn_lstm_ppo_epoch_update(*(ptrs or ok), *vals)
        return rc, lib.pedn_last_error(None).decode()

    for i in range(26):
        ptrs = list(ok)
        ptrs[i] = None
        rc, msg = call(ptrs)
        assert rc == -1 and "null" in msg, (i, rc, msg)
    for kw, word in (({"hidden": 32}, "hidden_size 64"), ({"layers": 2}, "one layer"), ({"T": 0}, "positive"), ({"N": 0}, "positive"),
                     ({"n_agents": 65536}, "positive"), ({"f64": 2}, "dtype flag"), ({"groups": 0}, "groups"), ({"groups": 65536}, "groups"),
                     ({"vpack": 8002}, "multiple of 4"), ({"apack": 0}, "empty"), ({"actor_lr": -1.0}, "lr"), ({"critic_lr": float("inf")}, "lr"),
                     ({"eps": float("nan")}, "eps"), ({"beta1": 1.0}, "betas"), ({"beta2": -0.5}, "betas"), ({"clip_eps": 0.0}, "clip_eps"),
                     ({"clip_eps": float("nan")}, "clip_eps"), ({"max_grad_norm": 0.0}, "max_grad_norm"),
                     ({"max_grad_norm": float("inf")}, "max_grad_norm"), ({"kl_tolerance": float("nan")}, "kl_tolerance")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    for i in range(7, 19):                                       # the packs, the workspace and the activations
        ptrs = list(ok)
        ptrs[i] = C.c_void_p(4096 + 256 * i + 4)
        rc, msg = call(ptrs)
        assert rc == -1 and "16-byte aligned" in msg, (i, rc, msg)
    assert lib.pedn_lstm_ppo_begin_update(None, 3, None) == -1 and "null" in lib.pedn_last_error(None).decode()
    assert lib.pedn_lstm_ppo_begin_update(C.c_void_p(4096), 0, None) == -1
