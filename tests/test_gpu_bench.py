"""bench.py end to end without --full: the line's contract (--steps timed steps, ms_per_step, value = rows / step time) and
--dump-outputs.  The inputs are seeded, so two runs hand back the same outputs up to rounding (the policy's calibration
times the first passes, so the kernels it picks may differ from run to run: the dense and the sparse path agree to ~1e-14)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 200_000


def _bench(tmp_path, name, steps):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--rows", str(ROWS), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout)               # stdout carries the line and nothing else
    return line, {p.stem: np.load(p) for p in out.iterdir()}


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    a, da = _bench(tmp_path, "a", 3)
    b, db = _bench(tmp_path, "b", 4)
    for line, steps in ((a, 3), (b, 4)):
        assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["config"]["rows_total"] == ROWS and line["unit"] == "samples/s" and line["higher_is_better"] is True
        assert abs(line["value"] - ROWS / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
        assert "roofline" not in line and "cpu_baseline" not in line
    assert set(da) == {"hn_alpha_vec", "hn_m_vecs", "hn_kappas", "hn_nus", "hn_w_mats", "hn_w_mats_inv", "ns", "x_bar_vecs",
                       "s_mats", "vl", "r_vecs"}
    for d in (da, db):
        assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in d.values())
        assert abs(d["ns"].sum() - ROWS) < 1e-9 * ROWS                    # the statistics of a pass over every row
        np.testing.assert_allclose(d["r_vecs"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert d["hn_w_mats"].shape == (64, 128, 128)
    # same inputs, one more iteration: the fit has moved on (the dump is of the LAST timed step) ...
    assert da["vl"][0] != db["vl"][0]
    # ... and a third run with --steps 3 gives back the first one's outputs
    c, dc = _bench(tmp_path, "c", 3)
    assert c["steps"] == 3
    for k in da:
        assert da[k].shape == dc[k].shape, k
        assert rel_err(dc[k], da[k]) < 1e-9, (k, rel_err(dc[k], da[k]))
