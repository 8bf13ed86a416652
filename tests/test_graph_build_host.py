"""CPU tests of the device graph build's C ABI (shd_pe_create_built,
shd_pe_graph_digest): declared in the header at ABI >= 10, exported and bound,
argument checks that need no device, and the ctypes mirror of ShdPeBuildInfo
against the compiler's layout."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from shdpe import generators as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "shd_pathengine.h")
NEW = ("shd_pe_create_built", "shd_pe_graph_digest")


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "shadow-1_amd")], check=True)
    from shdpe import engine
    return engine.load_library()


def test_header_declares_the_entry_points():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+SHD_PE_ABI_VERSION\s+(\d+)", txt).group(1)) >= 10
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
    for name, value in (("SHD_PE_BUILD_HOST", 0), ("SHD_PE_BUILD_DEVICE", 1), ("SHD_PE_BUILD_AUTO", 2)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, code).group(1)) == value
    assert "ShdPeBuildInfo" in code


def test_exported_and_listed(lib):
    from shdpe import engine
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "shadow-1_amd", "libshdpe.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", out))
    for s in NEW:
        assert s in exported and s in engine.EXPORTS and hasattr(lib, s), s
    assert (engine.BUILD_HOST, engine.BUILD_DEVICE, engine.BUILD_AUTO) == (0, 1, 2)


def test_build_kernels_are_in_the_code_object():
    data = open(os.path.join(ROOT, "shadow-1_amd", "libshdpe.so"), "rb").read()
    for k in (b"k_build_count", b"k_build_scan", b"k_build_scatter", b"k_build_rows", b"k_build_link",
              b"k_build_vfinal"):
        assert k in data, k


def test_unknown_graph_build_is_einval(lib):
    """Before any other work: no device is looked for, a null graph is not
    reached, and the info block is left alone."""
    from shdpe.engine import EINVAL, Engine, EngineError, BuildInfoC
    top = G.random_sparse(20, 3, seed=1)
    for bad in (7, -1, 3):
        with pytest.raises(EngineError) as ei:
            Engine(top, np.arange(20), graph_build=bad)
        assert ei.value.code == EINVAL
    info = BuildInfoC()
    info.built = 77
    h = ctypes.c_void_p()
    assert lib.shd_pe_create_built(None, None, 0, None, 7, ctypes.byref(info), ctypes.byref(h)) == EINVAL
    assert info.built == 77 and not h.value


def test_digest_argument_checks(lib):
    from shdpe.engine import EINVAL
    cnt = ctypes.c_int32(0)
    out = np.zeros(64, np.uint64)
    assert lib.shd_pe_graph_digest(None, 0, out.ctypes.data_as(ctypes.c_void_p), 64, ctypes.byref(cnt)) == EINVAL
    assert cnt.value == 64


def test_no_silent_host_run_without_a_device(lib):
    """The device build answers SHD_PE_ENODEV where no device is found; the host
    build of the new entry point stops at the same place as shd_pe_create."""
    import torch
    if torch.cuda.is_available():
        return
    from shdpe.engine import BUILD_AUTO, BUILD_DEVICE, BUILD_HOST, ENODEV, Engine, EngineError
    top = G.random_sparse(20, 3, seed=1)
    for build in (BUILD_HOST, BUILD_DEVICE, BUILD_AUTO):
        with pytest.raises(EngineError) as ei:
            Engine(top, np.arange(20), graph_build=build)
        assert ei.value.code == ENODEV, build


def test_auto_threshold_is_the_measured_one():
    """BUILD_AUTO_MIN_EDGES is the edge count the timing file derives, and that
    file's derivation gives it: the smallest complete graph from which on the
    device build's median beats the host build's by more than the spread."""
    import json
    src = open(os.path.join(ROOT, "shadow-1_amd", "csrc", "pe_build.hpp")).read()
    const = int(re.search(r"BUILD_AUTO_MIN_EDGES\s*=\s*(\d+)\s*;", src).group(1))
    prof = json.load(open(os.path.join(ROOT, "profiles", "create_device_build.json")))
    assert prof["auto_threshold_edges"] == const
    rows = sorted(prof["auto_threshold_derivation"]["shapes"], key=lambda r: r["edges"])
    for r in rows:
        assert r["device_wins"] == (r["device_median"] < r["host_median"] - r["spread"])
    wins = [r["edges"] for r in rows if all(q["device_wins"] for q in rows if q["edges"] >= r["edges"])]
    assert wins and min(wins) == const
    # C3a and C3b: the shapes the device build is for
    for shape in ("c3a", "c3b"):
        s = prof["shapes"][shape]
        assert s["device_built"] == 1 and s["device_handedOff"] == 0
        assert s["device_ms"]["max"] < s["host_ms"]["min"]


def test_staging_copy_under_sanitizers(tmp_path):
    """tests/native/stage_copy.cpp: the read-back's threaded copy out of a staging
    buffer (Stager::copy_out, host code only), -fsanitize=address,undefined in a
    stand-alone program."""
    import shutil
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "stage_copy")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "shadow-1_amd", "csrc"), os.path.join(ROOT, "tests", "native", "stage_copy.cpp"),
           "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lpthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("AddressSanitizer runtime unavailable")
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "stage_copy: 0 failures" in r.stdout and not r.stderr.strip(), \
        (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_build_info_layout_matches_binding(tmp_path):
    """sizeof and every field offset of ShdPeBuildInfo, from the C compiler."""
    from shdpe.engine import BuildInfoC
    fields = [f for f, _ in BuildInfoC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shd_pathengine.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(ShdPeBuildInfo));\n' +
                   "".join('  printf(" %%zu", offsetof(ShdPeBuildInfo, %s));\n' % f for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(BuildInfoC)
    assert got[1:] == [getattr(BuildInfoC, f).offset for f in fields]
