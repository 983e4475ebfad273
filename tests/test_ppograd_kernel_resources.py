"""The PPO epochs' kernels (pednstream_amd/csrc/pedn_ppo_grad.hpp) are exactly the ones below, none has scratch or spills, and their LDS
and VGPRs are within the figures of DESIGN section 20, read from the code object inside the built libpedn_hip.so (no GPU needed; same
reader as tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"ppograd_kernel", "ppograd_reduce_kernel", "ppograd_adam_kernel", "ppograd_begin_kernel"}
# the weight staging 64 x 33 words, the gathered input chunk 32 x 32, h1, h2, h3 and the LayerNorm's normalised rows (32 x 64 each), the
# output gradient 32 x 68, the heads' hand-over 32 x 16, two per-(row, action) areas 32 x 8 (the loss' elements), and four per-row areas
# of 32 (the LayerNorm's sqrt(var + eps), the value's gradient, the rows' t and e)
GRAD_LDS_BYTES = 4 * (64 * 33 + 32 * 32 + 4 * 32 * 64 + 32 * 68 + 32 * 16 + 2 * 32 * 8 + 4 * 32)
REDUCE_LDS_BYTES = 8 * 256          # the halving tree of sum g^2 in double
GRAD_VGPRS = 256                    # (58 624 bytes of LDS let two workgroups share a compute unit: 2 waves per SIMD, which leaves room for 256)
REDUCE_VGPRS = 32
ADAM_VGPRS = 64


def test_ppograd_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("ppograd")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        print(name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    assert GRAD_LDS_BYTES == 58624 and 2 * GRAD_LDS_BYTES <= 160 * 1024
    assert mine["ppograd_kernel"].get("group_segment_fixed_size", 0) == GRAD_LDS_BYTES
    assert mine["ppograd_reduce_kernel"].get("group_segment_fixed_size", 0) == REDUCE_LDS_BYTES
    assert mine["ppograd_adam_kernel"].get("group_segment_fixed_size", 0) == 0 and mine["ppograd_begin_kernel"].get("group_segment_fixed_size", 0) == 0
    assert mine["ppograd_kernel"]["vgpr_count"] <= GRAD_VGPRS
    assert mine["ppograd_reduce_kernel"]["vgpr_count"] <= REDUCE_VGPRS
    assert mine["ppograd_adam_kernel"]["vgpr_count"] <= ADAM_VGPRS
    # no existing resource test claims them: the kernels that start with ppo_ are pedn_ppo.hpp's
    assert {name for name in kernels if name.startswith("ppo_")} == {"ppo_eval_kernel"}
