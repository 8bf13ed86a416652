"""Time of the batched path extraction at the north-star shape: C4
(generators.make_config("c4"): 100,000 vertices, 16,384 attached), one request
per source, dst = att[(7919 * i + 1) % T] -- what topology.c:1831-1841 logs on
every first miss of a source.  One process, after compute_all:

  sizing    Engine.get_paths' first half alone (verts == NULL): lengths and
            statuses from the table, no emulation.
  batched   shd_pe_get_paths with verts / hopLat / hopRel: after a warm-up call,
            `--repeats` calls; per call its wall time and the device time of
            shd_pe_paths_info.  Once as the engine runs it (the batch tier
            first) and once, in a second engine, with SHDPE_PATHS_FAST=0 (every
            source by the grouped emulation); the two outputs must be equal
            byte for byte.
  loop      shd_pe_get_path, the one-pair call, over a 64-source sample of the
            same requests, scaled to T: the only way to these paths before.
            Its paths are checked equal to the batched call's before anything
            is written.

  python tools/paths_time.py [--config c4q] [--out profiles/paths_c4shape.json]

The per-row sparse and the dense mode (--config c2, --config c3b), whose fast
tier is the row tier (shd_pe_paths_set_row_tier), take another protocol: this
process starts one child per step, each under its own `timeout`, and starts
nothing more once a step has failed.

  rows      (with --row-tier) compute_all for scale, the sizing call, then the
            call with the row tier on: a warm-up, `--repeats` timed calls, the
            per-tier counters.
  emu       the same engine without the row tier, every source by the grouped
            emulation: all requests, or (--emu-sources N; 512 by default at c3b,
            where a full run takes minutes) those of the first N sources, scaled
            to all by the number of emulation groups.  Its bytes must equal the
            row tier's for the same requests.

  python tools/paths_time.py --config c2 --row-tier     -> profiles/paths_c2shape.json
  python tools/paths_time.py --config c3b --row-tier    -> profiles/paths_c3bshape.json
  SHDPE_LIB=<older build> python tools/paths_time.py --config c2 --out <file>   (emu alone)"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-1_amd"))


def _range(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


ROW_TIER_CONFIGS = ("c2", "c2q", "c3b", "c3bq")


def _digest(out, n):
    """sha256 of the output of the first n requests (paths lie in request order)."""
    offsets, verts, status, hl, hr = out
    e = int(offsets[n])
    h = hashlib.sha256()
    for a in (offsets[:n + 1], verts[:e], status[:n], hl[:e], hr[:e]):
        h.update(a.tobytes())
    return h.hexdigest()


def _requests(eng):
    import numpy as np
    T = eng.T
    src = eng.attached.copy()
    dst = eng.attached[(7919 * np.arange(T, dtype=np.int64) + 1) % T].astype(np.int32)
    return src, dst


def _timed_calls(eng, src, dst, what, repeats):
    wall, dev, out, info = [], [], None, None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = eng.get_paths(src, dst, hops=True)
        wall.append((time.perf_counter() - t0) * 1e3)
        info = eng.paths_info()
        dev.append(info["device_ms"])
        print(f"{what}: {wall[-1]:.1f} ms wall, {dev[-1]:.1f} ms device", file=sys.stderr, flush=True)
    return out, wall, dev, info


def step_rows(args):
    """Child: compute_all, sizing, the call with the row tier on."""
    import numpy as np
    from shdpe import engine as E
    from shdpe import generators as G
    top, att = G.make_config(args.config)
    eng = E.Engine(top, att)                 # raises without a gfx950 device: no fallback
    eng.reset_stats()
    eng.compute_all()
    st = eng.stats()
    T = eng.T
    src, dst = _requests(eng)
    lib = E.load_library()
    size_ms = []
    for _ in range(1 + max(5, args.repeats)):            # (the first: code object load)
        offsets = np.zeros(T + 1, np.int64)
        status = np.zeros(T, np.int32)
        o = E.PathsOutC(offsets.ctypes.data_as(C.c_void_p), None, None, None, status.ctypes.data_as(C.c_void_p), 0)
        t0 = time.perf_counter()
        rc = lib.shd_pe_get_paths(eng.h, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), T,
                                  C.byref(o))
        if rc:
            raise SystemExit(f"shd_pe_get_paths (sizing): {rc}")
        size_ms.append((time.perf_counter() - t0) * 1e3)
    eng.set_paths_row_tier(True)
    eng.get_paths(src, dst, hops=True)                   # warm-up
    out, wall, dev, info = _timed_calls(eng, src, dst, "row tier", args.repeats)
    lens = np.diff(out[0])
    n_emu = args.emu_sources if 0 < args.emu_sources < T else T
    res = {
        "mode": st["mode"], "vertices": int(top.n), "requests": int(T),
        "compute_all_ms": st["msTotal"], "rows_exact": st["rowsExact"], "rows_tie_early": st["rowsTieEarly"],
        "sizing_call_wall_ms": _range(size_ms[1:]),
        "row_tier_calls_timed": len(wall), "row_tier_wall_ms": _range(wall), "row_tier_device_ms": _range(dev),
        "sources_by_tier": {"rows": info["rows"], "tie": info["tie"], "emulated": info["emulated"],
                            "batch": info["batch"]},
        "requests_handed_on": info["handed_on"], "emulation_groups": info["groups"],
        "row_tier_over_compute_all": statistics.median(dev) / st["msTotal"] if st["msTotal"] else None,
        "path_entries": int(out[0][-1]), "path_vertices_mean": float(lens.mean()), "path_vertices_max": int(lens.max()),
        "digest_requests": n_emu, "digest": _digest(out, n_emu),
    }
    eng.close()
    with open(args.out, "w") as f:
        json.dump(res, f)


def step_emu(args):
    """Child: the grouped emulation alone, over all requests or a sample of sources."""
    from shdpe import engine as E
    from shdpe import generators as G
    top, att = G.make_config(args.config)
    eng = E.Engine(top, att)
    eng.reset_stats()
    eng.compute_all()
    st = eng.stats()
    T = eng.T
    src, dst = _requests(eng)
    n = args.emu_sources if 0 < args.emu_sources < T else T
    eng.get_paths(src[:2], dst[:2], hops=True)           # warm-up: code object load
    out, wall, dev, info = _timed_calls(eng, src[:n], dst[:n], f"emulation only, {n} sources",
                                        args.emu_repeats or (args.repeats if n == T else 1))
    if info["emulated"] != n or info["batch"] or info["tie"] or info.get("rows", 0):
        raise SystemExit(f"not the grouped emulation alone: {info}")
    per_group = -(-info["emulated"] // max(1, info["groups"]))
    scale = -(-T // per_group) / max(1, info["groups"])
    res = {
        "emulation_only_sources": int(n), "emulation_only_calls_timed": len(wall),
        "emulation_only_groups": info["groups"], "emulation_rows_per_group": int(per_group),
        "emulation_only_wall_ms": _range(wall), "emulation_only_device_ms": _range(dev),
        "emulation_only_scale_to_all": scale,
        "emulation_only_wall_ms_scaled": statistics.median(wall) * scale,
        "emulation_only_device_ms_scaled": statistics.median(dev) * scale,
        "emulation_compute_all_ms": st["msTotal"],
        "digest_requests": int(n), "digest": _digest(out, n),
        "library": "SHDPE_LIB" if os.environ.get("SHDPE_LIB") else "in-tree",
    }
    eng.close()
    with open(args.out, "w") as f:
        json.dump(res, f)


def run_steps(args):
    """This process opens no GPU: one child per step under its own time limit,
    in sequence, and nothing more after a step that failed."""
    steps = (["rows"] if args.row_tier else []) + ["emu"]
    res = {"config": args.config, "unit": "ms"}
    digests = {}
    for step in steps:
        part = f"{args.out}.{step}.part"
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               "--config", args.config, "--step", step, "--out", part, "--repeats", str(args.repeats),
               "--emu-repeats", str(args.emu_repeats), "--emu-sources", str(args.emu_sources)]
        rc = subprocess.run(cmd).returncode
        if rc:
            raise SystemExit(f"step {step}: exit status {rc}; no further step was started")
        with open(part) as f:
            got = json.load(f)
        os.remove(part)
        digests[step] = (got.pop("digest_requests"), got.pop("digest"))
        res.update(got)
    if len(digests) == 2:
        if digests["rows"] != digests["emu"]:
            raise SystemExit(f"the row tier and the grouped emulation alone differ: {digests}")
        res["bytes_equal_over_requests"] = digests["emu"][0]
        res["emulation_only_over_row_tier_wall"] = (res["emulation_only_wall_ms_scaled"] /
                                                    res["row_tier_wall_ms"]["median"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c4")
    ap.add_argument("--row-tier", action="store_true", help="c2 / c3b: time the call with the row tier on")
    ap.add_argument("--emu-sources", type=int, default=-1,
                    help="c2 / c3b: sources of the emulation-only call (0: all; default: all, 512 at c3b)")
    ap.add_argument("--step", choices=("rows", "emu"), default=None, help="(a child of the c2 / c3b protocol)")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds per step of the c2 / c3b protocol")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--emu-repeats", type=int, default=0, help="calls of the emulation-only engine (0: --repeats)")
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=None, help="default: profiles/paths_<config>shape.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", f"paths_{args.config}shape.json")
    if args.emu_sources < 0:
        args.emu_sources = 512 if args.config.startswith("c3") else 0
    if args.step:
        return step_rows(args) if args.step == "rows" else step_emu(args)
    if args.row_tier or args.config in ROW_TIER_CONFIGS:
        return run_steps(args)
    import numpy as np
    from shdpe import engine as E
    from shdpe import generators as G

    top, att = G.make_config(args.config)
    eng = E.Engine(top, att)                 # raises without a gfx950 device: no fallback
    eng.tune()
    eng.reset_stats()
    eng.compute_all()
    st = eng.stats()
    T = eng.T
    print(f"rows: {st['rowsComputed']} computed, {st['rowsExact']} exact, {st['rowsTieEarly']} early-stop tie",
          file=sys.stderr, flush=True)
    src = eng.attached.copy()
    dst = eng.attached[(7919 * np.arange(T, dtype=np.int64) + 1) % T].astype(np.int32)
    lib = E.load_library()

    def sizing():
        offsets = np.zeros(T + 1, np.int64)
        status = np.zeros(T, np.int32)
        o = E.PathsOutC(offsets.ctypes.data_as(C.c_void_p), None, None, None,
                        status.ctypes.data_as(C.c_void_p), 0)
        t0 = time.perf_counter()
        rc = lib.shd_pe_get_paths(eng.h, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                  T, C.byref(o))
        if rc:
            raise SystemExit(f"shd_pe_get_paths (sizing): {rc}")
        return (time.perf_counter() - t0) * 1e3, offsets

    def batched(e, what, repeats):
        out = e.get_paths(src, dst, hops=True)  # warm-up
        wall, dev, info = [], [], None
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = e.get_paths(src, dst, hops=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            info = e.paths_info()
            dev.append(info["device_ms"])
            print(f"{what}: {wall[-1]:.1f} ms wall, {dev[-1]:.1f} ms device", file=sys.stderr, flush=True)
        return out, wall, dev, info

    sizing()                                  # warm-up: code object load
    size_ms = [sizing()[0] for _ in range(max(5, args.repeats))]
    print(f"compute_all {st['msTotal']:.1f} ms, sizing {statistics.median(size_ms):.2f} ms", file=sys.stderr,
          flush=True)
    out, wall, dev, info = batched(eng, "batched call", args.repeats)
    offsets, verts, status = out[0], out[1], out[2]

    idx = np.linspace(0, T - 1, args.sample).astype(np.int64)
    eng.get_path(int(src[idx[0]]), int(dst[idx[0]]))     # warm-up
    eng.get_path(int(src[idx[1]]), int(dst[idx[1]]))     # (leaves another source cached)
    t0 = time.perf_counter()
    loop = [eng.get_path(int(src[i]), int(dst[i])) for i in idx]
    loop_ms = (time.perf_counter() - t0) * 1e3
    for j, i in enumerate(idx):
        if status[i] != 0 or verts[offsets[i]:offsets[i + 1]].tolist() != loop[j]:
            raise SystemExit(f"request {i}: the batched call and shd_pe_get_path differ")
    loop_scaled = loop_ms * T / args.sample
    lens = np.diff(offsets)
    eng.close()

    os.environ["SHDPE_PATHS_FAST"] = "0"
    eng = E.Engine(top, att, debug_flags=E.DEBUG_ENV)
    eng.compute_all()
    out0, wall0, dev0, info0 = batched(eng, "emulation only", args.emu_repeats or args.repeats)
    for a, b in zip(out, out0):
        if a.tobytes() != b.tobytes():
            raise SystemExit("the batch tier and the grouped emulation alone differ")

    res = {
        "config": args.config, "vertices": int(top.n), "requests": int(T), "unit": "ms",
        "compute_all_ms": st["msTotal"], "rows_exact": st["rowsExact"], "rows_tie_early": st["rowsTieEarly"], "exact_grid_rows_per_group": int(-(-info0["emulated"] // max(1, info0["groups"]))),
        "sizing_call_wall_ms": _range(size_ms),
        "batched_calls_timed": len(wall), "emulation_only_calls_timed": len(wall0),
        "batched_wall_ms": _range(wall), "batched_device_ms": _range(dev),
        "sources_by_tier": {"batch": info["batch"], "tie": info["tie"], "emulated": info["emulated"]},
        "requests_handed_on": info["handed_on"], "emulation_groups": info["groups"],
        "emulation_only_wall_ms": _range(wall0), "emulation_only_device_ms": _range(dev0),
        "emulation_only_groups": info0["groups"],
        "path_entries": int(offsets[-1]), "path_vertices_mean": float(lens.mean()), "path_vertices_max": int(lens.max()),
        "get_path_loop_sample": args.sample, "get_path_loop_sample_ms": loop_ms,
        "get_path_loop_scaled_ms": loop_scaled,
        "get_path_loop_over_batched_wall": loop_scaled / statistics.median(wall),
        "get_path_loop_over_emulation_only_wall": loop_scaled / statistics.median(wall0),
        "batched_over_compute_all": statistics.median(dev) / st["msTotal"] if st["msTotal"] else None,
        "compared_against": "a loop of shd_pe_get_path over a sample of the same requests on the same box, "
                            "scaled to all of them",
    }
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
