"""The running-normalisation kernel (pednstream_amd/csrc/pedn_norm.hpp) has no scratch: no private segment, no scratch access in its
code and no spill, read from the code object inside the built libpedn_hip.so (no GPU needed; same reader as
tests/test_kernel_resources.py)."""
from test_kernel_resources import kernel_metadata


def test_norm_kernel_has_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    mine = {name: k for name, k in kernels.items() if name.startswith("norm_")}
    assert set(mine) == {"norm_kernel"}, sorted(mine)
    for name, k in mine.items():
        assert k.get("private_segment_fixed_size", 0) == 0, (name, k)
        assert k.get("scratch_instructions", 0) == 0, (name, k)
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, (name, k)
