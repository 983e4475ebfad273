"""examples/ppo_lstm_full_update.py runs end to end on the GPU: rollout -> evaluate_store -> compute_gae -> the normalisation line ->
update_store, the epochs once eagerly and once as the replay of one captured graph, with no torch module."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ppo_lstm_full_update_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_lstm_full_update.py"), "nine_intersections", "16", "12", "3"],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-2000:])
    assert "nine_intersections x 16 envs, 3 recurrent agents: 12 rows (11 replayed steps), two updates of 3 epochs" in out.stdout, out.stdout[-1000:]
    assert "second update: steps" in out.stdout and "nan" not in out.stdout.lower(), out.stdout[-1000:]
