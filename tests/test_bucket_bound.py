"""The delta-stepping bucket bound (csrc/pe_bucket.hpp, used by k_sparse_rows'
two relax loops and k_batch_rows) on the host, under sanitizers: the checks
are in tests/native/bucket_bound.cpp.  This is the only test of the widths at
which the bound used to stall (delta < ulp(key)/2): no GPU test goes there.
Also the host side of shd_pe_sparse_info (ABI 15)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shadow-1_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
NEW = "shd_pe_sparse_info"


def test_bucket_bound_under_sanitizers(tmp_path):
    """Strictly above the key; the earlier formula's value wherever that was
    above the key, bit for bit; +inf for an infinite width; a sweep over n
    sorted keys ends within n advances."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bucket_bound")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(ROOT, "tests", "native", "bucket_bound.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("AddressSanitizer runtime unavailable")
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "OK" in r.stdout and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"pairs (\d+) stalls (\d+) step2 (\d+) stall14 (\d+) of (\d+) sweeps (\d+)", r.stdout)
    pairs, stalls, step2, stall14, n14, sweeps = map(int, m.groups())
    # every step of the bound was reached, and the stalling width stalls as often as measured
    # (delta = 1e-14, keys uniform in 1..1000: 78% of the keys)
    assert pairs > 10 ** 6 and stalls > 0 and step2 > 0 and sweeps >= 100
    assert 0.70 < stall14 / n14 < 0.86


def test_one_bound_in_the_kernels():
    """The header has no HIP include, and the kernels call it: no copy of the
    formula is left in the .hip files."""
    hdr = open(os.path.join(CSRC, "pe_bucket.hpp")).read()
    assert "#include" not in re.sub(r"//.*", "", hdr)
    uses = 0
    for f in ("pe_kernels.hip", "pe_batch.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert '#include "pe_bucket.hpp"' in src
        assert not re.search(r"floor\s*\(\s*\w+\s*/\s*delta\s*\)", src), f
        uses += len(re.findall(r"\bbucket_bound\(", src))
    assert uses == 3


def test_sparse_info_declared_exported_bound():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)", txt).group(1)) >= 15
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+ShdPe\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int64_t\s+\w+\[8\]\s*\)" % NEW, code)
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % NEW, txt, flags=re.S)
    assert m, "no comment in front of the declaration"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for word in ["out[%d]" % k for k in range(8)] + ["ABI 15", "replaces nothing in topology.c"]:
        assert word in doc, word
    so = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert NEW in set(re.findall(r"\bT (\w+)", out))
    assert NEW in engine.EXPORTS and hasattr(lib, NEW) and hasattr(engine.Engine, "sparse_info")
    # null arguments are refused before anything is touched
    buf = np.full(8, -7, np.int64)
    assert lib.shd_pe_sparse_info(None, 0, buf.ctypes.data) != 0
    assert lib.shd_pe_sparse_info(None, 0, None) != 0
    assert (buf == -7).all()
