"""Time of the link / vertex load reduction (shd_pe_path_load) at the north-star
shape: C4 (generators.make_config("c4"): 100,000 vertices, 16,384 attached),
after compute_all.  This process opens no GPU: every step is a child under its
own `timeout`, in sequence, and nothing more starts once a step has failed.

  a         the 16,384 requests of tools/paths_time.py (one per source), in one
            process through shd_pe_get_paths (vertices and hop attributes: the
            yardstick, code the load call does not touch) and through
            shd_pe_path_load: a warm-up call each, then `--repeats` timed calls;
            median / min / max of wall time and of shd_pe_paths_info's device
            time.  The load call's sums are checked against numpy over the
            get_paths output first.  Expectation: load device median <= get_paths
            device median + 2 * (get_paths max - min); both values are written.
  b         1,048,576 requests, 64 destinations for each source, shuffled: with
            the sort by source and with SHDPE_LOAD_SORT=0; for each, time and
            tier counters, and from a second engine with debug counters the
            global atomic adds issued per path entry.  All runs must give the
            same sums.
  variant   (with --variant-lib and / or --variant-env) leg b's sorted run again
            with another build of the library (SHDPE_LIB) and / or another debug
            switch: the A/B of a reduction kernel variant on one box, e.g.
              tools/build_variant.sh load_plain "" tools/variants/path_load_plain.patch
              python tools/path_load_time.py --variant-lib shadow-1_amd/libshdpe_load_plain.so \\
                     --variant-env SHDPE_LOAD_COMBINE=0
  c         (--leg-c) all T destinations for the first 1,024 sources.

  python tools/path_load_time.py [--out profiles/path_load_c4shape.json]"""
import argparse
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


def _engine(args, flags=0):
    from shdpe import engine as E
    from shdpe import generators as G
    top, att = G.make_config(args.config)
    eng = E.Engine(top, att, debug_flags=flags)     # raises without a gfx950 device: no fallback
    eng.tune()
    eng.reset_stats()
    eng.compute_all()
    return E, eng


def _requests_a(eng):
    import numpy as np
    T = eng.T
    src = eng.attached.copy()
    dst = eng.attached[(7919 * np.arange(T, dtype=np.int64) + 1) % T].astype(np.int32)
    return src, dst


def _requests_b(eng, per_source=64):
    import numpy as np
    T = eng.T
    i = np.repeat(np.arange(T, dtype=np.int64), per_source)
    j = np.tile(np.arange(per_source, dtype=np.int64), T)
    src = eng.attached[i]
    dst = eng.attached[(7919 * i + 1 + 257 * j) % T]
    p = np.random.default_rng(1).permutation(src.shape[0])
    return np.ascontiguousarray(src[p], np.int32), np.ascontiguousarray(dst[p], np.int32)


def _requests_c(eng, sources=1024):
    import numpy as np
    T = eng.T
    return np.repeat(eng.attached[:sources], T).astype(np.int32), np.tile(eng.attached, sources).astype(np.int32)


def _digest(out):
    h = hashlib.sha256()
    for k in ("arc", "vertex", "status", "totals"):
        h.update(out[k].tobytes())
    return h.hexdigest()


def _timed(call, info, what, repeats):
    call()                                           # warm-up
    wall, dev, out = [], [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(info()["device_ms"])
        print(f"{what}: {wall[-1]:.1f} ms wall, {dev[-1]:.1f} ms device", file=sys.stderr, flush=True)
    return out, wall, dev


def step_a(args):
    import numpy as np
    E, eng = _engine(args)
    st = eng.stats()
    src, dst = _requests_a(eng)
    paths, gw, gd = _timed(lambda: eng.get_paths(src, dst, hops=True), eng.paths_info, "get_paths", args.repeats)
    ginfo = eng.paths_info()
    load, lw, ld = _timed(lambda: eng.path_load(src, dst), eng.paths_info, "path_load", args.repeats)
    linfo = eng.paths_info()
    # the sums against numpy over the get_paths output
    offsets, verts, status = paths[0], paths[1].astype(np.int64), paths[2]
    af, at = eng.arcs()
    key = af.astype(np.int64) * eng.top.n + at
    vertex = np.zeros(eng.top.n, np.uint64)
    np.add.at(vertex, verts, np.uint64(1))
    first = np.zeros(verts.shape[0], bool)
    first[offsets[:-1][np.diff(offsets) > 0]] = True
    hop = np.flatnonzero(~first)
    k = verts[hop - 1] * eng.top.n + verts[hop]
    a = np.searchsorted(key, k)
    arc = np.zeros(key.shape[0], np.uint64)
    np.add.at(arc, a, np.uint64(1))
    if not (np.array_equal(key[a], k) and np.array_equal(arc, load["arc"]) and
            np.array_equal(vertex, load["vertex"]) and np.array_equal(status, load["status"])):
        raise SystemExit("shd_pe_path_load differs from the sums over shd_pe_get_paths' output")
    bound = statistics.median(gd) + 2.0 * (max(gd) - min(gd))
    tiers = ("batch", "tie", "emulated", "rows", "handed_on", "groups")
    res = {
        "a_requests": int(src.shape[0]), "a_path_entries": int(offsets[-1]), "compute_all_ms": st["msTotal"],
        "a_calls_timed": len(gw),
        "a_get_paths_wall_ms": _range(gw), "a_get_paths_device_ms": _range(gd),
        "a_path_load_wall_ms": _range(lw), "a_path_load_device_ms": _range(ld),
        "a_get_paths_info": {t: ginfo[t] for t in tiers}, "a_path_load_info": {t: linfo[t] for t in tiers},
        "a_expectation_bound_device_ms": bound,
        "a_expectation_holds": bool(statistics.median(ld) <= bound),
        "a_busiest_arc_load": int(load["arc"].max()), "a_busiest_vertex_load": int(load["vertex"].max()),
        "a_arcs_with_load": int(np.count_nonzero(load["arc"])), "arcs": int(key.shape[0]),
    }
    eng.close()
    return res


def _load_run(args, what, requests):
    """One engine for the timing, a second with debug counters for the atomics issued."""
    E, eng = _engine(args, flags=1)                  # SHD_PE_DEBUG_ENV: the child's SHDPE_* switches
    src, dst = requests(eng)
    out, wall, dev = _timed(lambda: eng.path_load(src, dst), eng.paths_info, what, args.repeats)
    info = eng.paths_info()
    eng.close()
    E, eng = _engine(args, flags=1 | E.DEBUG_COUNTERS)
    again = eng.path_load(src, dst)
    li = eng.path_load_info()
    eng.close()
    if _digest(again) != _digest(out):
        raise SystemExit(f"{what}: two engines give different sums")
    return {
        "requests": int(src.shape[0]), "path_entries": li["entries"], "calls_timed": len(wall),
        "wall_ms": _range(wall), "device_ms": _range(dev),
        "tier_passes": {t: info[t] for t in ("batch", "tie", "emulated", "rows")}, "emulation_groups": info["groups"],
        "requests_refused": int(out["totals"][3]),
        "global_atomics": li["atomics"], "global_atomics_per_entry": li["atomics"] / max(1, li["entries"]),
        "digest": _digest(out), "library": os.path.relpath(os.environ["SHDPE_LIB"], ROOT) if os.environ.get("SHDPE_LIB") else "in-tree",
        "switches": {k: v for k, v in os.environ.items() if k.startswith("SHDPE_LOAD_")},
    }


STEPS = {
    "a": step_a,
    "b_sorted": lambda args: {"b_sorted": _load_run(args, "b sorted", _requests_b)},
    "b_unsorted": lambda args: {"b_unsorted": _load_run(args, "b unsorted", _requests_b)},
    "b_variant": lambda args: {"b_variant": _load_run(args, "b variant", _requests_b)},
    "c": lambda args: {"c_first_1024_sources": _load_run(args, "c", _requests_c)},
}


def run_steps(args):
    plan = [("a", {}), ("b_sorted", {}), ("b_unsorted", {"SHDPE_LOAD_SORT": "0"})]
    if args.variant_lib or args.variant_env:
        env = dict(kv.split("=", 1) for kv in args.variant_env)
        if args.variant_lib:
            env["SHDPE_LIB"] = os.path.abspath(args.variant_lib)
        plan.append(("b_variant", env))
    if args.leg_c:
        plan.append(("c", {}))
    res = {"config": args.config, "unit": "ms"}
    for step, env in plan:
        part = f"{args.out}.{step}.part"
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               "--config", args.config, "--step", step, "--out", part, "--repeats", str(args.repeats)]
        rc = subprocess.run(cmd, env={**os.environ, **env}).returncode
        if rc:
            raise SystemExit(f"step {step}: exit status {rc}; no further step was started")
        with open(part) as f:
            res.update(json.load(f))
        os.remove(part)
    digests = {k: v["digest"] for k, v in res.items() if k.startswith("b_")}
    if len(set(digests.values())) != 1:
        raise SystemExit(f"the runs of leg b give different sums: {digests}")
    res["b_sums_equal"] = sorted(digests)
    res["b_unsorted_over_sorted_device"] = (res["b_unsorted"]["device_ms"]["median"] /
                                            res["b_sorted"]["device_ms"]["median"])
    if "b_variant" in res:
        res["b_variant_over_sorted_device"] = (res["b_variant"]["device_ms"]["median"] /
                                               res["b_sorted"]["device_ms"]["median"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c4")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(a child of the protocol)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--variant-lib", default=None, help="another build of the library for leg b's sorted run")
    ap.add_argument("--variant-env", action="append", default=[], metavar="NAME=VALUE",
                    help="a debug switch of that run (repeatable)")
    ap.add_argument("--leg-c", action="store_true", help="also all T destinations for the first 1,024 sources")
    ap.add_argument("--out", default=None, help="default: profiles/path_load_<config>shape.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", f"path_load_{args.config}shape.json")
    if args.step:
        res = STEPS[args.step](args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    run_steps(args)


if __name__ == "__main__":
    main()
