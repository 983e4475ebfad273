"""The recurrent PPO epochs' kernels (pednstream_amd/csrc/pedn_lstm_grad.hpp) are exactly the ones below, none has scratch or spills, and
their LDS and VGPRs are within the figures of DESIGN section 21, read from the code object inside the built libpedn_hip.so (no GPU needed;
same reader as tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"lstmgrad_seq_fwd_kernel", "lstmgrad_seq_bwd_kernel", "lstmgrad_dw_kernel", "lstmgrad_reduce_kernel", "lstmgrad_adam_kernel"}
# forward: lstm_seq_kernel's areas: the weight staging 256 x 33 words, the gathered input chunk 32 x 32, h and relu(h) (32 x 64 each), the
# heads' hand-over 32 x 16
FWD_LDS_BYTES = 4 * (256 * 33 + 32 * 32 + 2 * 32 * 64 + 32 * 16)
# backward: a of the tile's 32 rows (rows of 260 words), W_hh transposed (64 rows of 257), the heads' output gradient 32 x 16
BWD_LDS_BYTES = 4 * (32 * 260 + 64 * 257 + 32 * 16)
# weight gradients: a (32 x 260), the gathered chunk of x (32 x 32), h[t - 1] and relu(h') (32 x 64 each), a chunk of a weight gradient
# 64 x 33, the heads' output gradient 32 x 16, two per-(row, action) areas 32 x 8, the rows' t and e
DW_LDS_BYTES = 4 * (32 * 260 + 32 * 32 + 2 * 32 * 64 + 64 * 33 + 32 * 16 + 2 * 32 * 8 + 2 * 32)
REDUCE_LDS_BYTES = 8 * 256          # the halving tree of sum g^2 in double
# section 21's ceilings: what the build uses (192, 134, 78, 14, 38) rounded up to the next allocation granule of 8 registers
FWD_VGPRS = 192
BWD_VGPRS = 136
DW_VGPRS = 80
REDUCE_VGPRS = 16
ADAM_VGPRS = 40


def test_lstmgrad_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("lstmgrad")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        print(name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    lds = lambda n: mine[n].get("group_segment_fixed_size", 0)
    assert FWD_LDS_BYTES == 56320 and BWD_LDS_BYTES == 101120 and DW_LDS_BYTES == 66560
    assert 2 * FWD_LDS_BYTES <= 160 * 1024 and BWD_LDS_BYTES <= 160 * 1024 < 2 * BWD_LDS_BYTES and 2 * DW_LDS_BYTES <= 160 * 1024
    assert lds("lstmgrad_seq_fwd_kernel") == FWD_LDS_BYTES and lds("lstmgrad_seq_bwd_kernel") == BWD_LDS_BYTES
    assert lds("lstmgrad_dw_kernel") == DW_LDS_BYTES and lds("lstmgrad_reduce_kernel") == REDUCE_LDS_BYTES and lds("lstmgrad_adam_kernel") == 0
    assert mine["lstmgrad_seq_fwd_kernel"]["vgpr_count"] <= FWD_VGPRS
    assert mine["lstmgrad_seq_bwd_kernel"]["vgpr_count"] <= BWD_VGPRS
    assert mine["lstmgrad_dw_kernel"]["vgpr_count"] <= DW_VGPRS
    assert mine["lstmgrad_reduce_kernel"]["vgpr_count"] <= REDUCE_VGPRS
    assert mine["lstmgrad_adam_kernel"]["vgpr_count"] <= ADAM_VGPRS
    # the kernels of sections 17 and 20 keep their names: no kernel of this file starts with lstm_, ppo_ or ppograd
    assert not any(name.startswith(("lstm_", "ppo_", "ppograd")) for name in mine)
