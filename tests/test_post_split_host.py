"""Host-side checks of the post-split entry point (ABI 11): declared, exported,
bound; ShdPeStats is as it was (the split reports through its own call)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
NEW = "shd_pe_post_split_info"


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    return engine.load_library()


def test_header_declares_the_entry_point():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)", txt).group(1)) >= 11
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NEW, code)


def test_exported_and_bound(lib):
    from shdpe import engine
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")],
                         capture_output=True, text=True, check=True).stdout
    assert NEW in set(re.findall(r"\bT (\w+)", out))
    assert NEW in engine.EXPORTS and hasattr(lib, NEW)
    assert hasattr(engine.Engine, "post_split_info")
    # null arguments are refused before anything is touched
    assert lib.shd_pe_post_split_info(None, None, None, None) != 0


def test_stats_struct_is_unchanged(lib):
    from shdpe.engine import Stats
    assert len(Stats._fields_) == 30 and ctypes.sizeof(Stats) == 216
    assert Stats._fields_[-1][0] == "relaxCoopAborts"
    assert lib.shd_pe_stats_size() == 216


def test_kernel_parts_are_in_the_code_object():
    """The predecessor part (PART 5) and the label part (PART 6) of
    k_batch_rows<16, 6, false, .> are compiled in."""
    data = open(os.path.join(ROOT, "shadow-1_amd", "libshdpe.so"), "rb").read()
    assert b"k_batch_rowsILi16ELi6ELb0ELi5E" in data and b"k_batch_rowsILi16ELi6ELb0ELi6E" in data
