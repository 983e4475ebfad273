"""Register budget of dead_link_kernel, read from the code object inside the built libpedn_hip.so (no GPU needed), as
tests/test_kernel_resources.py does for the step kernels it lists.

The lean kernel pays off only as a short wave at full occupancy: built for 8 waves per SIMD (at most 64 vector registers), with no
spill of either kind -- a scalar spill would sit in front of the loads its few dependent steps wait for --, no scratch and no LDS."""
from test_kernel_resources import kernel_metadata


def test_dead_link_kernel_fits_eight_waves_without_spills(tmp_path):
    k = kernel_metadata(tmp_path)
    mine = {n: r for n, r in k.items() if n.startswith("dead_link_kernel")}
    assert len(mine) == 1, sorted(k)[:8]
    (name, r), = mine.items()
    print(name, r)
    assert r["vgpr_count"] <= 64, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r.get("scratch_instructions", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r
    assert r["group_segment_fixed_size"] == 0, r
