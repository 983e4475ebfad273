"""The replay kernels (pednstream_amd/csrc/pedn_replay.hpp) are exactly the ones below and none has scratch: no private segment, no
scratch access in its code and no spill, read from the code object inside the built libpedn_hip.so (no GPU needed; same reader as
tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"replay_push_kernel", "replay_sample_kernel"}


def test_replay_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("replay_")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    assert mine["replay_push_kernel"].get("group_segment_fixed_size", 0) == 0          # the gather's hand-over is the only LDS
    assert 0 < mine["replay_sample_kernel"].get("group_segment_fixed_size", 0) <= 256
