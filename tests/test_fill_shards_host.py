"""CPU test of the host half of shd_pe_fill_rowstore_shards (pe_fill.cpp):
need rounds, routing to the owning shards and the answers' way into the row
image, checked through the row store itself against plain
shd_rowstore_store calls (tests/native/fill_apply.cpp)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_need_rounds_routing_and_answers_under_sanitizers(tmp_path):
    """tests/native/fill_apply.cpp + pe_fill.cpp + pe_rowstore.cpp alone,
    -fsanitize=address,undefined: T in {1, 17, 65}, shard plans of 1 to 4
    owners with empty shards, ok and failed answers with and without a
    provisional direct entry, budgets down to one need per round."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fill_apply")
    csrc = os.path.join(ROOT, "shadow-1_amd", "csrc")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "native", "fill_apply.cpp"),
           os.path.join(csrc, "pe_fill.cpp"), os.path.join(csrc, "pe_rowstore.cpp"), "-pthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("AddressSanitizer runtime unavailable")
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK 144 cases") and not r.stderr.strip(), \
        (r.stdout, r.stderr[-3000:])
    assert int(r.stdout.split()[3]) >= 1000          # needs applied over all cases


def test_binding_mirrors_the_info_struct():
    """ShdPeFillShardsInfo field for field, as the header declares it."""
    import ctypes
    import re
    from shdpe.engine import FillShardsInfo
    txt = open(os.path.join(ROOT, "include", "shd_pathengine.h")).read()
    body = re.search(r"typedef struct ShdPeFillShardsInfo \{(.*?)\} ShdPeFillShardsInfo;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f for f, _ in FillShardsInfo._fields_]
    assert ctypes.sizeof(FillShardsInfo) == 2 * 4 + 4 * 8 + 4 * 8
