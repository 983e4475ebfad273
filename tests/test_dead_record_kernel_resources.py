"""Register budget of dead_link_kernel and dead_prep_kernel, read from the code object inside the built libpedn_hip.so (no GPU needed),
through tests/test_kernel_resources.py's reader.

dead_link_kernel takes its slot-uniform results from a record (DeadRec) that dead_prep_kernel fills: the wave is shorter than the one that
evaluated them itself, so it must need no more vector registers than that one did -- PARENT_VGPRS, the count of the kernel in the
build of the commit before the record -- and stay within the 64 of 8 waves per SIMD.  Neither kernel may use LDS or scratch or spill a
register of either kind: the lean kernel's share of a CU is set through LDS that it does not use (dead_lds_bytes), and the prep kernel
inlines send_flow and recv_flow whole."""
import pytest

from test_kernel_resources import kernel_metadata

PARENT_VGPRS = 42


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return kernel_metadata(tmp_path_factory.mktemp("dead_record"))


@pytest.mark.parametrize("kernel", ["dead_link_kernel", "dead_prep_kernel"])
def test_no_lds_no_scratch_no_spill(kernels, kernel):
    mine = {n: r for n, r in kernels.items() if n.startswith(kernel)}
    assert len(mine) == 1, sorted(kernels)[:8]
    (name, r), = mine.items()
    print(name, r)
    assert r["group_segment_fixed_size"] == 0, r
    assert r.get("scratch_instructions", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r


def test_dead_link_kernel_needs_no_more_vector_registers_than_before_the_record(kernels):
    (name, r), = [(n, r) for n, r in kernels.items() if n.startswith("dead_link_kernel")]
    print(name, r)
    assert r["vgpr_count"] <= 64, r
    assert r["vgpr_count"] <= PARENT_VGPRS, (r, PARENT_VGPRS)
