"""The SAC kernels (pednstream_amd/csrc/pedn_sac.hpp) are exactly the ones below and none has scratch: no private segment, no scratch
access in its code and no spill, read from the code object inside the built libpedn_hip.so (no GPU needed; same reader as
tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"sac_target_kernel", "sac_polyak_kernel"}
# per wave (3): a weight chunk 64 x 33 words, an input chunk 8 x 32, hidden rows 8 x 64; per critic wave (2): fc input rows 8 x 76;
# the heads' hand-over 8 x 16, next_action 8 x 8, logp 8 x 8, entropy 8, q1 and q2 2 x 8 words
LDS_BYTES = 4 * (3 * (64 * 33 + 8 * 32 + 8 * 64) + 2 * 8 * 76 + 8 * 16 + 8 * 8 + 8 * 8 + 8 + 2 * 8)
VGPRS = 125        # what sac_target_kernel took before its accumulation moved to pedn_mlp.hpp (3 waves per SIMD)


def test_sac_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("sac_")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        print(name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    assert 0 < mine["sac_target_kernel"].get("group_segment_fixed_size", 0) <= LDS_BYTES
    assert mine["sac_polyak_kernel"].get("group_segment_fixed_size", 0) == 0
    assert mine["sac_target_kernel"]["vgpr_count"] <= VGPRS
