"""examples/sac_replay.py runs end to end on the GPU: stacked policy, captured pushes, a minibatch and an update per agent and step."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sac_replay_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sac_replay.py"), "nine_intersections", "16", "60"], capture_output=True,
                         text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "60 policy steps pushed (59 replayed, 1 eager), 960 transitions" in out.stdout, out.stdout[-1000:]
    assert "states (64, 4, 15), actions (64, 3) float64, rewards (64,), next_states (64, 4, 15), dones (64,), idx (64, 2)" in out.stdout
    assert "next_states[:, :-1] == states[:, 1:] is True" in out.stdout
