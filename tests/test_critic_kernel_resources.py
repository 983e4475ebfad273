"""The critic kernels (pednstream_amd/csrc/pedn_critic.hpp) are exactly the ones below, none has scratch or spills, and their LDS and
VGPRs are within the figures of DESIGN section 18, read from the code object inside the built libpedn_hip.so (no GPU needed; same reader
as tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"critic_grad_kernel", "critic_adam_kernel"}
# per critic (2): staging rows 64 x 33 words, h1 32 x 64, the fc input rows 32 x 96, h3 / the output gradient 32 x 68, q - td and its
# gradient 2 x 32; the gathered input chunk 32 x 32 once
LDS_BYTES = 4 * (2 * (64 * 33 + 32 * 64 + 32 * 96 + 32 * 68 + 2 * 32) + 32 * 32)
GRAD_VGPRS = 132       # (8 waves of one workgroup on 4 SIMDs: 2 waves per SIMD, which leaves room for 256)
ADAM_VGPRS = 59


def test_critic_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("critic_")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        print(name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    assert LDS_BYTES == 79872 and 0 < mine["critic_grad_kernel"].get("group_segment_fixed_size", 0) <= LDS_BYTES
    assert mine["critic_adam_kernel"].get("group_segment_fixed_size", 0) == 0
    assert mine["critic_grad_kernel"]["vgpr_count"] <= GRAD_VGPRS
    assert mine["critic_adam_kernel"]["vgpr_count"] <= ADAM_VGPRS
