"""The per-(batch, lane) bucket key offsets of pe_plan.cpp (lane_offsets, and
batch_order_cost handing them out with the batches) on the host, under
sanitizers: the checks are in tests/native/lane_offsets.cpp, the graphs those
of tests/plan_cost_cases.py at 8 and 16 lanes."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from plan_cost_cases import plan_cost_graphs
from test_plan_cost import write_graph


def test_lane_offsets_under_sanitizers(tmp_path):
    """Finite, >= 0, batch minimum exactly 0, pads 0, one-lane batches 0, a
    batch with an unreached lane exactly rowOff, the same on 1 and 16 planner
    threads and under lane permutations, exact on dyadic synthetic distances,
    blind to a common constant and to empty groups; batch_order_cost still
    returns every position once, and its offsets are those of its batches."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "shadow-1_amd", "csrc")
    exe = str(tmp_path / "lane_offsets")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "lane_offsets.cpp"), os.path.join(csrc, "pe_plan.cpp"),
           os.path.join(csrc, "pe_graph.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("AddressSanitizer runtime unavailable")
    assert b.returncode == 0, b.stderr[-2000:]
    dirs = []
    for name, top, att in plan_cost_graphs():
        dirs.append(str(tmp_path / name))
        write_graph(dirs[-1], top, att)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe] + dirs, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "OK" in r.stdout and not r.stderr.strip(), (r.stdout, r.stderr[-3000:])
    # the graphs reached every kind of batch the checks are about
    tally = {k: 0 for k in ("least-squares", "fallback", "one-lane", "padded")}
    lines = [ln for ln in r.stdout.splitlines() if " attached " in ln]
    assert len(lines) == len(dirs) and any(" directed 1 " in ln for ln in lines)
    for ln in lines:
        for k in tally:
            tally[k] += int(re.search(rf" {k} (\d+)", ln).group(1))
    assert all(v > 0 for v in tally.values()), tally
