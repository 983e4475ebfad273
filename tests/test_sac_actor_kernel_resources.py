"""The SAC actor step's kernels (pednstream_amd/csrc/pedn_actor_grad.hpp) are exactly the ones below, none has scratch or spills, and
their LDS and VGPRs are within the figures of DESIGN section 19, read from the code object inside the built libpedn_hip.so (no GPU needed;
same reader as tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"sacactor_grad_kernel", "sacactor_adam_kernel"}
# three staging areas of 64 x 33 words, the gathered input chunk 32 x 32, h1 of the three networks and the actor's h2 and h3 (32 x 64 each),
# the critics' fc input rows 2 x 32 x 96, three areas of 32 x 68 (the critics' fc outputs, the actor's output gradient), the heads' hand-over
# 32 x 16, five per-(row, action) areas 32 x 8 (new_action, logp, std, eps, t), the rows' entropy, q1, q2 and two loss terms (5 x 32), the
# critics' fc_out weights 2 x 64; d q / d action 2 x 8 doubles
LDS_BYTES = 4 * (3 * 64 * 33 + 32 * 32 + 5 * 32 * 64 + 2 * 32 * 96 + 3 * 32 * 68 + 32 * 16 + 5 * 32 * 8 + 5 * 32 + 2 * 64) + 8 * 2 * 8
GRAD_VGPRS = 168       # (12 waves of one workgroup on 4 SIMDs: 3 waves per SIMD, which leaves room for 168)
ADAM_VGPRS = 51


def test_sac_actor_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("sacactor_")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        print(name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    assert LDS_BYTES == 129536 and LDS_BYTES <= 160 * 1024
    assert 0 < mine["sacactor_grad_kernel"].get("group_segment_fixed_size", 0) <= LDS_BYTES
    assert mine["sacactor_adam_kernel"].get("group_segment_fixed_size", 0) == 0
    assert mine["sacactor_grad_kernel"]["vgpr_count"] <= GRAD_VGPRS
    assert mine["sacactor_adam_kernel"]["vgpr_count"] <= ADAM_VGPRS
