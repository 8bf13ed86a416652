"""bench.py on the GPU: a plain run times the headline only and, with
--dump-outputs, writes the rows the timed path left in the table -- the same
rows, bit for bit, that an engine built in this process computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from shdpe import generators as G

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("cpu_baseline", "cpu_baseline_all_cores", "speedup_vs_cpu", "host_fill", "secondary",
             "tie_stress", "d2h")


# c1: 183 rows, all of them fit the dump (contiguous read); c2: 10,000 rows
# of 10,000 targets, the dump is a seeded sample (row-by-row read)
@pytest.mark.parametrize("workload,sampled", [("c1", False), ("c2", True)])
def test_plain_run_line_and_dumped_rows(workload, sampled, tmp_path):
    from shdpe.engine import Engine
    steps = 3
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--workload", workload, "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "source rows/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    T = out["config"]["sources"]
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(T / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in out], out.keys()
    assert "stream_GBps" not in out["roofline"]

    want_dtype = {"rows": np.float64, "lat": np.float64, "rel": np.float64, "hops": np.float32,
                  "flags": np.float32, "pred": np.float64}
    assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in want_dtype)
    got = {k: np.load(d / (k + ".npy")) for k in want_dtype}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    pos = got["rows"].astype(np.int64)
    assert np.all(np.diff(pos) > 0) and pos[0] >= 0 and pos[-1] < T
    assert (pos.shape[0] < T) == sampled
    for k, dt in want_dtype.items():
        assert got[k].dtype == dt
        if k != "rows":
            assert got[k].shape == (pos.shape[0], T)

    top, att = G.make_config(workload)
    eng = Engine(top, att)
    eng.compute_all()
    for i, p in enumerate(pos):
        row = eng.get_rows(int(p), 1)
        for k in ("lat", "rel"):
            assert np.array_equal(row[k][0].view(np.int64), got[k][i].view(np.int64)), (k, p)
        for k in ("hops", "flags", "pred"):
            assert np.array_equal(row[k][0].astype(np.float64), got[k][i].astype(np.float64)), (k, p)
    eng.close()
