"""CPU tests of the parent tier's dense form at the C ABI: the header's
parent-tier text names the dense mode and no longer excludes it, the ABI
version stays 16 with the addition listed under it, the vertex-id instantiation
of the reduction kernel is in the library's gfx950 code object, and the setter
refuses a NULL engine without touching a GPU."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
LIB = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")


@pytest.fixture(scope="module")
def E():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    engine.load_library()
    return engine


def _parent_tier_text():
    """The comment above ShdPeTableLoadIn from 'A fourth route' on, on one line."""
    raw = open(HEADER).read()
    m = re.search(r"A fourth route, the parent tier.*?\*/\s*typedef struct ShdPeTableLoadIn", raw, flags=re.S)
    assert m
    return re.sub(r"\s*\n\s*\*\s*", " ", m.group(0))


def test_header_names_the_dense_mode():
    txt = _parent_tier_text()
    assert "dense mode is served from the predecessor pass's parent rows" in txt
    assert "not in the dense mode" not in txt
    assert "forceMode 3" in txt and "folded latencies" in txt          # what it still excludes


def test_abi_stays_16_with_the_addition_listed():
    raw = open(HEADER).read()
    ver = re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)\s*/\*(.*?)\*/", raw, flags=re.S)
    assert int(ver.group(1)) == 16
    later = re.findall(r"later under 16:([^;]*?)(?:;|$)", ver.group(2), flags=re.S)
    assert len(later) >= 2
    assert any("dense mode" in x for x in later)
    assert not re.search(r"\b17\s*:", ver.group(2))


def test_vertex_id_kernel_built_for_gfx950():
    """Both instantiations of k_tree_load_parents<PAR> (0: in-arc words, 1: vertex
    ids) by their mangled names."""
    data = open(LIB, "rb").read()
    assert b"gfx950" in data
    assert re.search(rb"19k_tree_load_parentsILi1EE", data)
    assert re.search(rb"19k_tree_load_parentsILi0EE", data)


def test_null_engine_is_einval(E):
    lib = E.load_library()
    assert lib.shd_pe_table_load_set_parent_tier(None, 1) == E.EINVAL
    assert lib.shd_pe_table_load_set_parent_tier(None, 0) == E.EINVAL


def test_python_docstrings_name_the_dense_mode(E):
    assert "dense mode" in E.Engine.set_table_load_parent_tier.__doc__
    assert "dense mode" in E.Engine.table_load_info.__doc__
    assert set(re.findall(r'"(\w+)": ', open(os.path.join(ROOT, "shadow-1_amd", "shdpe", "engine.py")).read()
                          .split("def table_load_info")[1].split("def ")[0])) == {
        "tree", "direct", "route", "handed_on", "claimed", "device_ms", "rounds", "atomics", "parents", "tie",
        "parent_claimed", "parent_atomics"}
