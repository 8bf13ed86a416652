"""batch_order_cost on the host is the reference of the device plan: its
batches, costs and lane offsets on the graphs of tests/device_plan_cases.py
must be those recorded in tests/golden/plan_order_cost.txt before the plan
kernels were added (tests/native/plan_order_cost.cpp prints one line of hashes
per graph, lane count, offset kind and position set)."""
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from device_plan_cases import ba1200, two_components, twins
from shdpe import generators as G
from test_plan_cost import write_graph


def test_host_plan_is_what_it_was(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "shadow-1_amd", "csrc")
    exe = str(tmp_path / "plan_order_cost")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "plan_order_cost.cpp"), os.path.join(csrc, "pe_plan.cpp"),
           os.path.join(csrc, "pe_graph.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("AddressSanitizer runtime unavailable")
    assert b.returncode == 0, b.stderr[-2000:]
    cases = {"ba1200": (ba1200(), G.sample_attached(1200, 300, seed=2)), "two_components": two_components(),
             "twins": twins()}
    args = []
    for name, (top, att) in cases.items():
        write_graph(str(tmp_path / name), top, att)
        args.append(f"{name}={tmp_path / name}")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout, r.stderr[-3000:])
    with open(os.path.join(GOLDEN, "plan_order_cost.txt")) as f:
        want = f.read()
    assert r.stdout == want
