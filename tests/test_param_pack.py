"""The parameter packs' shared helper (pednstream_amd/packs.py) on its own, without a GPU: the layout of networks in one float32 tensor,
the views, and what loading and binding refuse.  policy.py, sac.py and ppo.py build their packs with it; their own host tests pin
the layouts the kernels read."""
import numpy as np
import pytest

from pednstream_amd import packs

F = np.float32
# sizes 13, 9 and 4: the networks behind the first two need padding, the one behind the third does not
NETS = [[("a.weight", (3, 4)), ("a.bias", (1,))], [("a.weight", (2, 4)), ("a.bias", (1,))], [("w", (4,))], [("a.weight", (1, 5)), ("a.bias", (2,))]]


def test_every_network_starts_on_a_multiple_of_4_floats():
    offsets, total = packs.layout(NETS)
    assert [list(cur) for cur in offsets] == [[k for k, _ in net] for net in NETS]
    end, used = 0, np.zeros(total, dtype=np.int32)
    for net, cur in zip(NETS, offsets):
        at = start = cur[net[0][0]][0]
        assert start % 4 == 0 and 0 <= start - end < 4                  # the next multiple of 4
        for key, shape in net:
            assert cur[key] == (at, shape)                               # the tensors lie one behind the other, in the list's order
            used[at:at + int(np.prod(shape))] += 1
            at += int(np.prod(shape))
        end = at
    assert [cur[net[0][0]][0] for net, cur in zip(NETS, offsets)] == [0, 16, 28, 32]
    assert used.max() == 1 and end == 39 and total == 40                 # rounded up
    assert packs.layout(NETS, round_total=False) == (offsets, 39)        # the actors' total is the last tensor's end
    assert packs.layout([]) == ([], 0)


def test_two_networks_per_agent_as_for_the_critics():
    from pednstream_amd import sac

    agents = [(0, 4, 0, 1), (5, 40, 1, 8), (45, 5, 9, 2)]
    per_agent = [sac.critic_shapes(ow, aw, 5) for (_, ow, _, aw) in agents]
    flat, total = packs.layout([shapes for shapes in per_agent for _ in range(2)])
    offsets, total2 = sac.critic_pack_layout(agents, 5)
    assert total == total2 and total % 4 == 0
    assert offsets == [flat[2 * i:2 * i + 2] for i in range(len(agents))]
    size = lambda shapes: sum(int(np.prod(s)) for _, s in shapes)
    at = 0
    for pair, shapes in zip(offsets, per_agent):
        for cur in pair:                                                 # critic 1, then critic 2 of the agent, each on the next multiple of 4
            assert cur["encoder.fc1.weight"][0] == -(-at // 4) * 4
            at = cur["encoder.fc1.weight"][0] + size(shapes)
            assert cur["fc_out.bias"] == (at - 1, (1,))


def test_views_load_and_repoint():
    torch = pytest.importorskip("torch")
    offsets, total = packs.layout(NETS)
    pack = torch.zeros(total)
    calls = []
    get = lambda: calls.append(1) or pack
    packs.load(offsets[1], {"a.weight": np.arange(8, dtype=np.float64).reshape(2, 4), "a.bias": torch.tensor([8.0], dtype=torch.float64)}, get)
    want = np.zeros(total, dtype=F)
    want[16:25] = np.arange(9)
    assert np.array_equal(pack.numpy(), want) and calls == [1]           # arrays and tensors, as float32, and nothing beside them
    v = packs.views(pack, offsets[1])
    assert list(v) == ["a.weight", "a.bias"] and tuple(v["a.weight"].shape) == (2, 4) and v["a.weight"].data_ptr() == pack[16:].data_ptr()
    m = torch.nn.Module()
    m.a = torch.nn.Linear(4, 2)
    m.a.bias = torch.nn.Parameter(torch.zeros(1))                        # (the network's shapes; never called)
    packs.check_module(m, offsets[1])
    assert packs.repoint(m, v) is m and m.a.weight.data_ptr() == pack[16:].data_ptr() and m.a.bias.data_ptr() == pack[24:].data_ptr()
    with torch.no_grad():
        m.a.weight.add_(1.0)                                             # what an optimiser's step does
    assert np.array_equal(pack.numpy()[16:24], np.arange(8) + 1)


def test_refusals_keep_their_texts():
    torch = pytest.importorskip("torch")
    offsets, total = packs.layout(NETS)

    def never():
        raise AssertionError("the pack is not touched before the state dict is accepted")

    with pytest.raises(ValueError) as e:
        packs.load(offsets[0], {"a.weight": np.zeros((3, 4), F), "b": np.zeros(1, F)}, never)
    assert str(e.value) == "state dict keys ['a.weight', 'b'] do not match ['a.bias', 'a.weight']"
    with pytest.raises(ValueError) as e:
        packs.load(offsets[0], {"a.weight": np.zeros((3, 4), F)}, never)
    assert str(e.value) == "state dict keys ['a.weight'] do not match ['a.bias', 'a.weight']"
    with pytest.raises(ValueError) as e:
        packs.load(offsets[0], {"a.weight": np.zeros((4, 3), F), "a.bias": np.zeros(1, F)}, never)
    assert str(e.value) == "a.weight: expected shape (3, 4), got (4, 3)"
    with pytest.raises(ValueError) as e:
        packs.check_module(torch.nn.Linear(2, 2), offsets[0], "critic_1: ")
    assert str(e.value) == "critic_1: the module's parameters ['bias', 'weight'] do not match ['a.bias', 'a.weight']"
    with pytest.raises(ValueError) as e:
        packs.index(["a", "b"], "c")
    assert str(e.value) == "Unknown agent: c" and packs.index(["a", "b"], "b") == 1
    for bad, text in ((None, "x must be a torch tensor"), (torch.zeros(2, 3), "x must be on cuda:0")):
        with pytest.raises(ValueError) as e:
            packs.check_tensor("x", bad, 0, (2, 3))
        assert str(e.value) == text
