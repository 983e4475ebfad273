"""examples/sac_critic_update.py runs end to end on the GPU: TD targets, the critic step and the Polyak update on the device, the actor and
alpha steps in torch on the bound modules."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sac_critic_update_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sac_critic_update.py"), "nine_intersections", "16", "24"],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "24 policy steps (23 replayed), 4 updates of 64 rows: 4 critic steps on the device, 4 target launches drew noise" in out.stdout, out.stdout[-1000:]
    assert "losses finite: True" in out.stdout, out.stdout[-1000:]
