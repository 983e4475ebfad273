"""examples/sac_full_update.py runs end to end on the GPU: the whole SAC update (TD targets, the critic step, the actor and temperature
step, the Polyak update) as replays of one captured graph, with no torch module."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sac_full_update_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sac_full_update.py"), "nine_intersections", "16", "24"],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    # the warm call with the steps switched off draws once, every replay once more
    assert ("24 policy steps (23 replayed), 4 updates of 64 rows in one captured graph: 4 critic steps and 4 actor steps on the device, "
            "5 actor launches drew noise") in out.stdout, out.stdout[-1000:]
    assert "all finite: True" in out.stdout and "moved by 0.00e+00" not in out.stdout, out.stdout[-1000:]
