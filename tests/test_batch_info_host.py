"""Host-side checks of the batch-round entry point (ABI 12): declared with a
comment that says what it replaces, exported, bound; the two test-only
switches are read with the other SHDPE_* variables, under SHD_PE_DEBUG_ENV."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
CSRC = os.path.join(ROOT, "shadow-1_amd", "csrc")
NEW = "shd_pe_batch_info"


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    return engine.load_library()


def test_header_declares_the_entry_point():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)", txt).group(1)) >= 12
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+ShdPe\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int64_t\s+\w+\[4\]\s*\)" % NEW, code)
    # the comment in front of it: the four values, and that topology.c has no counterpart
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % NEW, txt, flags=re.S)
    assert m, "no comment in front of the declaration"
    doc = " ".join(m.group(1).replace("*", " ").split())
    for word in ("out[0]", "out[1]", "out[2]", "out[3]", "shd_pe_reset_stats", "shd_pe_get_paths", "shd_pe_tune"):
        assert word in doc, word
    assert "replaces nothing in topology.c" in doc


def test_exported_and_bound(lib):
    from shdpe import engine
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")],
                         capture_output=True, text=True, check=True).stdout
    assert NEW in set(re.findall(r"\bT (\w+)", out))
    assert NEW in engine.EXPORTS and hasattr(lib, NEW)
    assert hasattr(engine.Engine, "batch_info")
    # null arguments are refused before anything is touched
    buf = np.full(4, -7, np.int64)
    assert lib.shd_pe_batch_info(None, 0, buf.ctypes.data) != 0
    assert lib.shd_pe_batch_info(None, 0, None) != 0
    assert (buf == -7).all()


def test_switches_are_read_under_debug_env_only():
    """SHDPE_BATCH_ROUND and SHDPE_TIE_SLOTS sit in read_tuning behind its
    SHD_PE_DEBUG_ENV return, and their Tuning fields default to `unchanged`."""
    src = open(os.path.join(CSRC, "pe_engine.hip")).read()
    body = re.search(r"static void read_tuning\(.*?\n}\n", src, flags=re.S).group(0)
    gate = body.index("if (!(flags & SHD_PE_DEBUG_ENV)) return;")
    for var, field in (("SHDPE_BATCH_ROUND", "batchRoundCap"), ("SHDPE_TIE_SLOTS", "tieSlotsCap")):
        m = re.search(r'gi\("%s",\s*t\.%s\);' % (var, field), body)
        assert m and m.start() > gate, var
        assert len(re.findall(r'"%s"' % var, src)) == 1, var       # read nowhere else
    dev = open(os.path.join(CSRC, "pe_device.hpp")).read()
    assert re.search(r"int\s+batchRoundCap\s*=\s*0\s*;\s*//\s*tests only", dev)
    assert re.search(r"int\s+tieSlotsCap\s*=\s*-1\s*;\s*//\s*tests only", dev)
