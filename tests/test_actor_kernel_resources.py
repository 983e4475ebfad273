"""The actor kernels (pednstream_amd/csrc/pedn_actor.hpp) are exactly the ones below and none has scratch: no private segment, no
scratch access in its code and no spill, read from the code object inside the built libpedn_hip.so (no GPU needed; same reader as
tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"actor_forward_kernel"}
# weight chunk 64 x 33 words + input chunk 32 x 32 + hidden rows 32 x 64 + head hand-over 32 x 16 words
LDS_BYTES = 4 * (64 * 33 + 32 * 32 + 32 * 64 + 32 * 16)
VGPRS = 140        # what the kernel took before its layers moved to pedn_mlp.hpp (3 waves per SIMD): sharing code costs no register


def test_actor_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("actor_")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        print(name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    assert 0 < mine["actor_forward_kernel"].get("group_segment_fixed_size", 0) <= LDS_BYTES
    assert mine["actor_forward_kernel"]["vgpr_count"] <= VGPRS
