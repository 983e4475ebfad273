"""Parameter packs of the RL kernels: the networks of every agent lie one behind the other in ONE float32 tensor, each network's tensors
in ``nn.Linear`` layout in the order the kernel walks them, every network on a multiple of 4 floats.  What ``policy.py`` (the actors),
``sac.py`` (the critics, two per agent) and ``ppo.py`` (the value networks) share: the layout, the views, loading and binding of
modules, the validation of a launch's tensors and the encoder of the modules beside the kernels."""
import numpy as np


def layout(networks, round_total=True):
    """(offsets, total) of ``networks`` = [[(state_dict key, shape)]]: offsets[n] = {key: (offset in floats, shape)}, the tensors of a
    network one behind the other, every network on a multiple of 4 floats; total (the pack's length) is rounded up to one on request."""
    offsets, at = [], 0
    for shapes in networks:
        at = -(-at // 4) * 4
        cur = {}
        for key, shape in shapes:
            cur[key] = (at, shape)
            at += int(np.prod(shape))
        offsets.append(cur)
    return offsets, -(-at // 4) * 4 if round_total else at


def index(agent_ids, agent_id):
    try:
        return agent_ids.index(agent_id)
    except ValueError:
        raise ValueError(f"Unknown agent: {agent_id}") from None


def views(pack, want):
    """{key: tensor} of the network ``want`` (an entry of ``layout``'s offsets) in ``nn.Linear`` shapes; the tensors ALIAS ``pack``."""
    return {k: pack[at:at + int(np.prod(shape))].view(*shape) for k, (at, shape) in want.items()}


def load(want, state_dict, pack):
    """Copy a network's tensors (torch tensors or arrays) into its views of ``pack()``, which is not called before their keys and
    shapes are found to be ``want``'s."""
    import torch

    keys = {k: v for k, v in state_dict.items()}
    if set(keys) != set(want):
        raise ValueError(f"state dict keys {sorted(keys)} do not match {sorted(want)}")
    for k, (_, shape) in want.items():
        if tuple(keys[k].shape) != tuple(shape):
            raise ValueError(f"{k}: expected shape {tuple(shape)}, got {tuple(keys[k].shape)}")
    dst = views(pack(), want)
    with torch.no_grad():
        for k, v in keys.items():
            dst[k].copy_(torch.as_tensor(np.asarray(v, dtype=np.float32)) if not isinstance(v, torch.Tensor) else v.detach().to(torch.float32))


def check_module(module, want, prefix=""):
    """Refuse a module whose parameters are not the network's."""
    params = dict(module.named_parameters())
    if set(params) != set(want):
        raise ValueError(f"{prefix}the module's parameters {sorted(params)} do not match {sorted(want)}")


def repoint(module, dst):
    """Point every ``param.data`` of a module whose parameters were loaded at its view in ``dst``: an optimiser that steps the module
    updates what the kernels read, with no copy per update."""
    for k, p in module.named_parameters():
        p.data = dst[k]
    return module


def check_tensor(name, t, device, shape, dtypes=None):
    """Refuse what a launch cannot read: ``t`` is a contiguous tensor on cuda:``device`` of ``shape`` and one of ``dtypes`` (float32)."""
    import torch

    dtypes = dtypes or (torch.float32,)
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    if not t.is_cuda or t.device.index != device:
        raise ValueError(f"{name} must be on cuda:{device}")
    if t.dtype not in dtypes or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {' or '.join(str(d).replace('torch.', '') for d in dtypes)} tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


def make_encoder(obs_w, stack_size, hidden_size=64):
    """The reference's stacked encoder (fc1, fc2, a ReLU behind each) on the flattened stack: input f * S + s is x[b, s, f]."""
    import torch
    from torch import nn

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2 = nn.Linear(int(stack_size) * int(obs_w), hidden_size), nn.Linear(hidden_size, hidden_size)

        def forward(self, x):
            return torch.relu(self.fc2(torch.relu(self.fc1(x))))

    return Encoder()
