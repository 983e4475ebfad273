"""Register budget of lean_block_kernel -- the dead links' block of steps per launch -- read from the code object inside the built
libpedn_hip.so (no GPU needed), through tests/test_kernel_resources.py's reader.

The block kernel keeps a lane's running sum, its previous receiving flow and the block's travel_time[t - 1 - W] values in registers and
unrolls its steps in full, so it needs more registers than dead_link_kernel; it must still fit the 64 of 8 waves per SIMD, use no LDS of
its own (its share of a CU is set through LDS that it does not use), no scratch and spill no register of either kind.  dead_link_kernel,
which still performs every block of one step, keeps the entry it had before the block kernel stood next to it."""
import pytest

from test_kernel_resources import kernel_metadata

# dead_link_kernel in the build of the commit before the block kernel
DEAD_LINK_KERNEL_BEFORE = {"group_segment_fixed_size": 0, "private_segment_fixed_size": 0, "sgpr_count": 70, "sgpr_spill_count": 0, "vgpr_count": 24,
                           "vgpr_spill_count": 0, "scratch_instructions": 0}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return kernel_metadata(tmp_path_factory.mktemp("dead_block"))


def test_one_block_kernel_within_eight_waves_without_lds_scratch_or_spill(kernels):
    mine = {n: r for n, r in kernels.items() if n.startswith("lean_block_kernel")}
    assert len(mine) == 1, sorted(kernels)[:8]
    (name, r), = mine.items()
    print(name, r)
    assert r["vgpr_count"] <= 64, r
    assert r["group_segment_fixed_size"] == 0, r
    assert r.get("scratch_instructions", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r


def test_dead_link_kernel_is_unchanged(kernels):
    (name, r), = [(n, r) for n, r in kernels.items() if n.startswith("dead_link_kernel")]
    print(name, r)
    assert r == DEAD_LINK_KERNEL_BEFORE, (r, DEAD_LINK_KERNEL_BEFORE)
