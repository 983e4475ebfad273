"""The block cutter of a split range (pedn_plan::dead_block_len, pednstream_amd/csrc/pedn_plan.hpp) without a GPU: its stand-alone driver
(tests/block_prog.cpp), built with AddressSanitizer + UBSan as tests/test_step_plan_host.py builds the planner's, cuts every range
t < t1 <= 64 for every block length K <= 16 and window W <= 16.

A block is one launch of lean_block_kernel: step t' of it reads travel_time[t' - 1 - W] and writes travel_time[t' - 1].  The kernel issues
those loads in front of its first store, so a block must never read a row that it writes itself."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MAX, K_MAX, W_MAX = 64, 16, 16


@pytest.fixture(scope="module")
def cuts(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("block")), "block_prog")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "block_prog.cpp")], check=True)
    r = subprocess.run([exe, str(T_MAX), str(K_MAX), str(W_MAX)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]          # the sanitizers stayed silent
    lines = r.stdout.splitlines()
    assert lines[0] == "max 16"          # one bit per step in the kernel's two 32-bit gate masks, PEDN_DEAD_BLOCK_MAX
    return [tuple(map(int, line.split())) for line in lines[1:]]


def test_every_range_is_cut_into_blocks_that_never_read_their_own_rows(cuts):
    assert len(cuts) == (T_MAX - 1) * T_MAX // 2 * K_MAX * W_MAX
    seen = set()
    for t, t1, K, W, *blocks in cuts:
        assert sum(blocks) == t1 - t, (t, t1, K, W, blocks)
        assert all(1 <= n <= min(K, W) for n in blocks), (t, t1, K, W, blocks)
        for n in blocks:
            written = range(t - 1, t + n - 1)                  # travel_time rows of the block's steps t .. t + n - 1
            read = range(t - 1 - W, t + n - 1 - W)             # ... and the rows they read W back (negative: the window has not filled)
            assert max(read) < min(written), (t, t1, K, W, blocks)
            t += n
        # as few launches as the two limits allow: every block but the last is full
        assert all(n == min(K, W) for n in blocks[:-1]), (t1, K, W, blocks)
        seen.add((len(blocks), blocks[0], blocks[-1]))
    assert {n for _, n, _ in seen} == set(range(1, 17)) and max(k for k, _, _ in seen) == T_MAX - 1 and (1, 1, 1) in seen
