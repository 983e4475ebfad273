"""The LSTM kernels (pednstream_amd/csrc/pedn_lstm.hpp) are exactly the ones below and have no scratch: no private segment, no scratch
access in their code and no spill, read from the code object inside the built libpedn_hip.so (no GPU needed; same reader as
tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata

KERNELS = {"lstm_actor_kernel", "lstm_reset_kernel", "lstm_seq_kernel"}
# the sum the kernels' comment derives: a weight chunk of the 256 gate rows x 33 words, an input chunk 32 x 32, the state rows h and the
# rows relu(h') the heads read 2 x 32 x 64, the heads' hand-over 32 x 16
LDS_BYTES = 4 * (256 * 33 + 32 * 32 + 2 * 32 * 64 + 32 * 16)
VGPRS = 256        # the budget of the 2 waves per SIMD both kernels declare (what their LDS leaves room for)


def test_lstm_kernels_have_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("lstm_")}
    assert set(mine) == KERNELS, sorted(mine)
    for name, k in mine.items():
        print(name, k)
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
    for name in ("lstm_actor_kernel", "lstm_seq_kernel"):
        assert mine[name].get("group_segment_fixed_size", 0) == LDS_BYTES == 56320, name
        assert mine[name]["vgpr_count"] <= VGPRS, name
        assert 2 * LDS_BYTES <= 160 * 1024 < 3 * LDS_BYTES                 # two workgroups per CU, as the cap assumes
    assert mine["lstm_reset_kernel"].get("group_segment_fixed_size", 0) == 0
