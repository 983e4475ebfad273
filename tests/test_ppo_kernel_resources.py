"""The PPO evaluation kernel (pednstream_amd/csrc/pedn_ppo.hpp) is exactly the one below and has no scratch: no private segment, no scratch
access in its code and no spill, read from the code object inside the built libpedn_hip.so (no GPU needed; same reader as
tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"ppo_eval_kernel"}
# the sum the kernel's comment derives: a weight chunk 64 x 33 words, an input chunk 32 x 32, hidden rows 32 x 64, the heads' hand-over
# 32 x 16, the tile's time rows and envs 2 x 32 words
LDS_BYTES = 4 * (64 * 33 + 32 * 32 + 32 * 64 + 32 * 16 + 2 * 32)
VGPRS = 128        # the kernel's cap (4 waves per SIMD), which it took in full before its layers moved to pedn_mlp.hpp


def test_ppo_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("ppo_")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        print(name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    assert 0 < mine["ppo_eval_kernel"].get("group_segment_fixed_size", 0) <= LDS_BYTES == 23040
    assert mine["ppo_eval_kernel"]["vgpr_count"] <= VGPRS
