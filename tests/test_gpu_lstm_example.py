"""examples/ppo_lstm_update.py runs end to end on the GPU: a captured rollout of the stateful LSTM actors, the values, next values and old
log-probabilities of its rows in one launch, TD targets and GAE from them, and one epoch of the clipped loss on bound modules."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ppo_lstm_update_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_lstm_update.py"), "nine_intersections", "16", "12"], capture_output=True,
                         text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "nine_intersections x 16 envs, 3 agents: 12 rows (11 replayed steps) of the LSTM actors, 1 epoch of the clipped loss" in out.stdout, out.stdout[-1000:]
    assert "values (12, 16, 3), next_values (12, 16, 3), old_log_probs (12, 16, 10)" in out.stdout
    # the epoch starts at ratio 1 (the evaluated distribution is the acting one); behind the optimiser steps the next launch differs
    ratio = re.search(r"mean ratio ([0-9.]+)", out.stdout)
    assert ratio and abs(float(ratio.group(1)) - 1) < 1e-3, out.stdout[-1000:]
    moved = re.search(r"after the epoch: mean \|log-prob - old\| ([0-9.e+-]+)", out.stdout)
    assert moved and 0 < float(moved.group(1)) < 1, out.stdout[-1000:]
