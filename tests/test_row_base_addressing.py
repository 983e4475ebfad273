"""History-row addressing of the node kernels, read from the disassembly of the built libpedn_hip.so (no GPU needed).

A node-kernel launch whose step index the host knows carries the start of every history row its waves address at a shared row
(DevView.rb, filled by row_bases in pedn_hip.hip); a wave adds its column's element offset.  Before, every access recomputed
((row * cols + col) * RS + r0) * size + base in 64-bit scalar arithmetic, and each of those 64-bit multiplies shows in the code as
an s_mul_hi_u32 / s_mul_hi_i32.  The headline instantiation (melbourne x 1024, owner-wave plan) held 76 of them at commit ea7478c;
the data-dependent look-backs, the demand row and the turning-fraction rows keep a few.

The clocked instantiations take their step from the device clock and keep the in-kernel arithmetic: their counts are pinned to what
the same command gave at commit ea7478c, so an edit of the shared step function that leaks into them shows here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pednstream_amd", "csrc", "libpedn_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"

HEADLINE = "node_kernel<false, false, false, 6, true, false, false>"
HEADLINE_MAX = 38      # half of the 76 at commit ea7478c
# s_mul_hi_u32 + s_mul_hi_i32 of every clocked instantiation <PR, LP, HIST, MD, LU, TF, CLK = true> at commit ea7478c
CLOCKED = {
    "node_kernel<false, false, false, 6, false, false, true>": 52,
    "node_kernel<false, false, false, 8, false, false, true>": 56,
    "node_kernel<false, false, true, 6, false, false, true>": 69,
    "node_kernel<false, false, true, 8, false, false, true>": 73,
    "node_kernel<true, false, false, 6, false, false, true>": 47,
    "node_kernel<true, false, false, 8, false, false, true>": 51,
    "node_kernel<true, false, true, 6, false, false, true>": 64,
    "node_kernel<true, false, true, 8, false, false, true>": 68,
}


def scalar_mul_hi(tmp_path):
    """kernel (demangled, without 'void' and the argument list) -> number of s_mul_hi_u32 + s_mul_hi_i32 in its code"""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools) or not os.path.exists(LIB) or not shutil.which("c++filt"):
        pytest.skip("ROCm LLVM tools, c++filt or the built library are not here")
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", LIB], check=True)
    subprocess.run([tools[1], "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    dis = subprocess.run([tools[2], "-d", co], check=True, capture_output=True, text=True).stdout
    counts, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1)
            counts.setdefault(cur, 0)
        elif cur is not None and re.match(r"^\s+s_mul_hi_[ui]32\s", line):
            counts[cur] += 1
    names = list(counts)
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r"\(.*", "", d).replace("void ", ""): counts[n] for n, d in zip(names, out)}


def test_headline_node_kernel_addresses_rows_from_the_launch_table(tmp_path):
    k = scalar_mul_hi(tmp_path)
    assert HEADLINE in k, sorted(n for n in k if n.startswith("node_kernel<"))[:8]
    print(f"{HEADLINE}: {k[HEADLINE]} s_mul_hi (76 at ea7478c, at most {HEADLINE_MAX})")
    assert k[HEADLINE] <= HEADLINE_MAX, k[HEADLINE]


def test_clocked_node_kernels_keep_their_in_kernel_addressing(tmp_path):
    k = scalar_mul_hi(tmp_path)
    got = {n: k.get(n) for n in CLOCKED}
    print(got)
    assert got == CLOCKED
