"""Host side of PPO's clipped-loss epochs (pednstream_amd/ppo.py: epoch_update, epoch_gradients, update_store, begin_update): the entry
points, the workspace's shape and every refusal that needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from pednstream_amd import engine, ppo
from pednstream_amd.policy import StackedActors
from pednstream_amd.rollout import RolloutStore

AGENTS = [(0, 4, 0, 1), (5, 56, 1, 8), (61, 6, 9, 2)]       # (obs0, obs_w, act0, act_w); the second one starts on an odd column
S = 5


def make():
    actors = StackedActors("ppo", AGENTS, low=np.zeros(11), high=np.full(11, 4.0), n_envs=1, n_obs=67, n_actions=11, stack_size=S)
    return ppo.PpoTargets(actors)


def test_the_entry_points_are_declared_behind_the_existing_ones():
    assert engine.ABI_VERSION == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pedn.h")).read()
    assert "int pedn_ppo_epoch_update(const float* obs" in header and "int pedn_ppo_begin_update(int32_t* stop_flags" in header
    assert engine.EXPORTS[-2:] == ["pedn_ppo_epoch_update", "pedn_ppo_begin_update"]      # additions, behind what was there
    assert engine.EXPORTS.index("pedn_ppo_epoch_update") > engine.EXPORTS.index("pedn_sac_actor_update")


def test_workspace_shape_is_bounded_by_the_groups():
    t = make()
    apack = t.actors.pack_size
    assert apack == sum(64 * S * ow + 64 + 2 * (64 * 64 + 64) + 128 + 2 * (64 * aw + aw) for (_, ow, _, aw) in AGENTS) + 2      # 2: the padding behind agent 0
    vpack = t.pack_size
    assert vpack == sum(-(-(64 * S * ow + 64 + 2 * (64 * 64 + 64) + 65) // 4) * 4 for (_, ow, _, _) in AGENTS)
    stride = -(-apack // 4) * 4 + vpack + 8 * 3
    assert stride % 4 == 0
    assert [t.update_workspace_shape(R, g) for (R, g) in ((1, 1), (32, 3), (33, 3), (97, 2), (97, 3), (97, 64), (700 * 2048, None))] == \
        [(1, stride), (1, stride), (2, stride), (2, stride), (3, stride), (4, stride), (ppo.DEFAULT_GROUPS, stride)]
    assert ppo.DEFAULT_GROUPS == 512 and ppo.TILE == 32
    # a whole rollout of 700 x 2048 rows needs no more than the default number of slabs: megabytes, not tiles x pack
    assert ppo.DEFAULT_GROUPS * stride * 4 < 2 ** 28 and (700 * 2048 // 32) * stride * 4 > 2 ** 33      # 185 MiB against 15.8 GiB
    with pytest.raises(ValueError, match="rows"):
        t.update_workspace_shape(0)
    assert ppo.SCALARS == ("actor_loss", "critic_loss", "approx_kl", "actor_norm", "value_norm", "actor_coef", "value_coef")


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
    obs, act, old = torch.zeros(T + 1, N, 67), torch.zeros(T, N, 11), torch.zeros(T, N, 11)
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
        with pytest.raises(ValueError, match="groups"):
            t.update_workspace_shape(64, bad)
    for bad in (None, np.zeros((T + 1, N, 67), dtype=np.float32), torch.zeros(N, 67), torch.zeros(1, N, 67)):
        with pytest.raises(ValueError, match="obs must"):
            t.epoch_update(bad, act, old, adv, td)
    with pytest.raises(ValueError, match="obs must be on cuda"):
        t.epoch_update(*args)                                   # CPU tensors
    with pytest.raises(ValueError, match="obs must be on cuda"):
        t.epoch_gradients(*args)
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
        t.update_store(fake_store(t, n_obs=66), old, adv, td)
    with pytest.raises(ValueError, match="epoch_update\\(\\) has not run"):
        t.epoch_outputs
    with pytest.raises(ValueError, match="Unknown agent"):
        t.adam_state(7, "actor")
    with pytest.raises(ValueError, match="which must be"):
        t.adam_state(0, "critic")
    assert t._udev is None and t._dev is None and t.actors._dev is None      # nothing above touched a device


def test_refusals_at_the_c_abi():
    lib = engine.lib()
    ok = [C.c_void_p(4096 + 256 * i) for i in range(25)]      # never read: every call below is refused before a launch
    tail = [10000, 8000, 3, 2, S, 67, 11, 3, 64, 0, 4, 1e-3, 10.0, 3e-4, 6e-4, 0.2, 0.5, 0.01, 0.9, 0.999, 1e-8, 1, None]

    def call(ptrs=None, **kw):
        names = ["apack", "vpack", "T", "N", "S", "n_obs", "n_actions", "n_agents", "hidden", "f64", "groups", "min_std", "max_std", "actor_lr",
                 "critic_lr", "clip_eps", "max_grad_norm", "kl_tolerance", "beta1", "beta2", "eps", "do_adam", "stream"]
        vals = list(tail)
        for k, v in kw.items():
            vals[names.index(k)] = v
        rc = lib.pedn_ppo_epoch_update(*(ptrs or ok), *vals)
        return rc, lib.pedn_last_error(None).decode()

    for i in [i for i in range(25) if i != 21]:              # (21: the optional tail outputs)
        ptrs = list(ok)
        ptrs[i] = None
        rc, msg = call(ptrs)
        assert rc == -1 and "null" in msg, (i, rc, msg)
    for kw, word in (({"hidden": 32}, "hidden_size 64"), ({"T": 0}, "positive"), ({"N": 0}, "positive"), ({"n_agents": 65536}, "positive"),
                     ({"f64": 2}, "dtype flag"), ({"groups": 0}, "groups"), ({"groups": 65536}, "groups"), ({"vpack": 8002}, "multiple of 4"),
                     ({"apack": 0}, "empty"), ({"actor_lr": -1.0}, "lr"), ({"critic_lr": float("inf")}, "lr"), ({"eps": float("nan")}, "eps"),
                     ({"beta1": 1.0}, "betas"), ({"beta2": -0.5}, "betas"), ({"clip_eps": 0.0}, "clip_eps"), ({"clip_eps": float("nan")}, "clip_eps"),
                     ({"max_grad_norm": 0.0}, "max_grad_norm"), ({"max_grad_norm": float("inf")}, "max_grad_norm"),
                     ({"kl_tolerance": float("nan")}, "kl_tolerance")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    for i in (7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17):        # the packs and the workspace
        ptrs = list(ok)
        ptrs[i] = C.c_void_p(4096 + 256 * i + 4)
        rc, msg = call(ptrs)
        assert rc == -1 and "16-byte aligned" in msg, (i, rc, msg)
    assert lib.pedn_ppo_begin_update(None, 3, None) == -1 and "null" in lib.pedn_last_error(None).decode()
    assert lib.pedn_ppo_begin_update(C.c_void_p(4096), 0, None) == -1
