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

  python tools/paths_time.py [--config c4q] [--out profiles/paths_c4shape.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shadow-1_amd"))


def _range(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c4")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--emu-repeats", type=int, default=0, help="calls of the emulation-only engine (0: --repeats)")
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=None, help="default: profiles/paths_<config>shape.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", f"paths_{args.config}shape.json")
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
