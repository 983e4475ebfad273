"""pedn_create refuses a faulty model description before it touches the device (pedn_compile.hpp: validate + compile run in front of
hipSetDevice and of the handle), with the message each fault always had; the intact model then creates and steps as ever."""
import numpy as np
import pytest

import compile_model as cm
from golden_util import ALL_FIELDS

pytestmark = pytest.mark.gpu

R = 128


def test_faulty_models_are_refused_and_the_intact_one_runs():
    from pednstream_amd.engine import Engine

    m = cm.model("nine_intersections")
    for kind in ("involution", "pair_ent", "ent_link"):
        bad, msg = cm.corrupt(m, kind)
        with pytest.raises(RuntimeError) as ei:
            Engine(bad, n_replicas=R, seed=5)
        assert str(ei.value) == f"pedn_create failed ({cm.PEDN_E_ARG}): {msg}", kind
    runs = []
    for _ in range(2):
        e = Engine(m, n_replicas=R, seed=5)
        e.run(1, 11)
        runs.append([e.read_block(fid, 0, 11) for fid in range(len(ALL_FIELDS))])
        flags = e.error_flags()
        assert flags[0] == 0
        e.close()
    for name, a, b in zip(ALL_FIELDS, *runs):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert float(runs[0][2].sum()) > 0          # cumulative_inflow: pedestrians have entered
