"""Batch order 2 on the host: hub-group distances, the source order and the
cost-ordered batch sequence of pe_plan.cpp, under sanitizers (the checks are
in tests/native/plan_cost.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from plan_cost_cases import plan_cost_graphs


def write_graph(d, top, att):
    os.makedirs(d)
    with open(os.path.join(d, "meta.txt"), "w") as f:
        f.write(f"{top.n} {int(top.directed)} {int(top.vloss is not None)}\n")
    top.src.astype(np.int32).tofile(os.path.join(d, "from.i32"))
    top.dst.astype(np.int32).tofile(os.path.join(d, "to.i32"))
    top.latency.astype(np.float64).tofile(os.path.join(d, "lat.f64"))
    top.loss.astype(np.float64).tofile(os.path.join(d, "loss.f64"))
    if top.vloss is not None:
        top.vloss.astype(np.float64).tofile(os.path.join(d, "vloss.f64"))
    np.asarray(att, np.int32).tofile(os.path.join(d, "att.i32"))


def test_batch_plan_cost_under_sanitizers(tmp_path):
    """Every position once and pads last, batch costs non-increasing, the same
    output on 1 and 16 threads, the lane offset the minimum over the groups
    (and order 1's offset), group distances against one Dijkstra per hub."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "shadow-1_amd", "csrc")
    exe = str(tmp_path / "plan_cost")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "plan_cost.cpp"), os.path.join(csrc, "pe_plan.cpp"),
           os.path.join(csrc, "pe_graph.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("AddressSanitizer runtime unavailable")
    assert b.returncode == 0, b.stderr[-2000:]
    dirs = []
    for name, top, att in plan_cost_graphs():
        assert len(att) % 8 != 0
        dirs.append(str(tmp_path / name))
        write_graph(dirs[-1], top, att)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe] + dirs, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "OK" in r.stdout and not r.stderr.strip(), (r.stdout, r.stderr[-3000:])
    assert " directed 1 " in r.stdout and r.stdout.count(" attached ") == len(dirs)
