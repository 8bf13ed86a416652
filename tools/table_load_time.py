"""Time of the all-pairs load call (shd_pe_table_load) at the north-star shape:
C4 (generators.make_config("c4"): 100,000 vertices, 16,384 attached), after
tune and compute_all.  This process opens no GPU: every step is a child under
its own `timeout`, in sequence, and nothing more starts once a step has failed.
Each step: one warm-up call, then `--repeats` timed calls; median / min / max
of wall time and of the call's device time.

  a         rows [0, 1024) with a seeded random weight matrix, tree tier on
  b         the same call with SHDPE_TLOAD_TREE=0: every source by the request route
  c         shd_pe_path_load on the same 16.8 M requests (the call there was
            before this one: tools/path_load_time.py's leg c with weights)
  d         all rows with weight == NULL, beside compute_all of the same process
  e         (--leg-e) all rows with a matrix, in blocks of `--block` rows made
            one at a time, so the matrix is never in host memory as a whole
  counters  (--counters) leg a with SHD_PE_DEBUG_COUNTERS: the commit's global
            adds per claimed tree entry
  once      (--step once, for a profiler: one call of leg d, nothing timed)

(a), (b) and (c) must give identical sums (sha256 over arc, vertex and totals,
kept in the file); (a) is expected below (b) and (c) by more than the sum of
their min-max spreads, and the file says whether it is.

  python tools/table_load_time.py [--out profiles/table_load_c4shape.json]"""
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


def _weights(rows, T, seed=1):
    import numpy as np
    return np.random.default_rng(seed).integers(0, 2 ** 40, (rows, T), endpoint=True).astype(np.uint64)


def _digest(out):
    h = hashlib.sha256()
    for k in ("arc", "vertex", "totals"):
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


def _result(eng, out, wall, dev, extra=None):
    info = eng.table_load_info()
    res = {"calls_timed": len(wall), "wall_ms": _range(wall), "device_ms": _range(dev),
           "info": {k: info[k] for k in ("tree", "direct", "route", "handed_on", "claimed", "rounds", "atomics")},
           "totals": [int(x) for x in out["totals"]], "digest": _digest(out),
           "switches": {k: v for k, v in os.environ.items() if k.startswith("SHDPE_TLOAD_")}}
    res.update(extra or {})
    return res


def _rows(args, eng):
    return min(args.sources, eng.T)


def step_table(args, what, flags=1):
    E, eng = _engine(args, flags=flags)              # SHD_PE_DEBUG_ENV: the child's SHDPE_* switches
    rows = _rows(args, eng)
    w = _weights(rows, eng.T)
    out, wall, dev = _timed(lambda: eng.table_load(0, rows, w), eng.table_load_info, what, args.repeats)
    res = _result(eng, out, wall, dev, {"sources": rows, "requests": rows * eng.T})
    eng.close()
    return res


def step_c(args):
    import numpy as np
    E, eng = _engine(args, flags=1)
    rows = _rows(args, eng)
    w = _weights(rows, eng.T).reshape(-1)
    src, dst = np.repeat(eng.attached[:rows], eng.T).astype(np.int32), np.tile(eng.attached, rows).astype(np.int32)
    out, wall, dev = _timed(lambda: eng.path_load(src, dst, w), eng.paths_info, "c", args.repeats)
    res = {"calls_timed": len(wall), "wall_ms": _range(wall), "device_ms": _range(dev), "sources": rows,
           "requests": int(src.shape[0]), "path_entries": eng.path_load_info()["entries"],
           "totals": [int(x) for x in out["totals"]], "digest": _digest(out)}
    eng.close()
    return res


def step_d(args):
    E, eng = _engine(args, flags=1)
    st = eng.stats()
    out, wall, dev = _timed(lambda: eng.table_load(), eng.table_load_info, "d", args.repeats)
    res = _result(eng, out, wall, dev, {"sources": eng.T, "requests": eng.T * eng.T, "compute_all_ms": st["msTotal"]})
    eng.close()
    return res


def step_e(args):
    import numpy as np
    E, eng = _engine(args, flags=1)
    T = eng.T

    def call():
        total = None
        for lo in range(0, T, args.block):
            n = min(args.block, T - lo)
            part = eng.table_load(lo, n, _weights(n, T, seed=lo + 1))
            call.dev += eng.table_load_info()["device_ms"]
            total = part if total is None else {k: total[k] + part[k] for k in part}
        return total
    call.dev = 0.0

    def info():
        dev, call.dev = call.dev, 0.0
        return {"device_ms": dev}
    call()
    info()
    wall, dev, out = [], [], None
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(info()["device_ms"])
        print(f"e: {wall[-1]:.1f} ms wall (weights made inside), {dev[-1]:.1f} ms device", file=sys.stderr, flush=True)
    res = {"calls_timed": len(wall), "wall_ms_with_weight_generation": _range(wall), "device_ms": _range(dev),
           "sources": T, "block_rows": args.block, "totals": [int(x) for x in out["totals"]], "digest": _digest(out)}
    assert int(out["totals"][1]) == int(np.sum(out["vertex"], dtype=np.uint64))
    eng.close()
    return res


def step_once(args):
    E, eng = _engine(args, flags=1)
    eng.table_load()
    info = eng.table_load_info()
    eng.close()
    return {"info": info}


STEPS = {
    "a": lambda args: {"a_tree": step_table(args, "a")},
    "b": lambda args: {"b_route": step_table(args, "b")},
    "c": lambda args: {"c_path_load": step_c(args)},
    "d": lambda args: {"d_all_rows_unit_weight": step_d(args)},
    "e": lambda args: {"e_all_rows_matrix": step_e(args)},
    "counters": lambda args: {"a_counters": step_table(args, "counters", flags=1 | 2)},
    "once": step_once,
}


def run_steps(args):
    plan = [("a", {}), ("b", {"SHDPE_TLOAD_TREE": "0"}), ("c", {}), ("d", {})]
    if args.leg_e:
        plan.append(("e", {}))
    if args.counters:
        plan.append(("counters", {}))
    res = {"config": args.config, "unit": "ms"}
    for step, env in plan:
        part = f"{args.out}.{step}.part"
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__),
               "--config", args.config, "--step", step, "--out", part, "--repeats", str(args.repeats),
               "--sources", str(args.sources), "--block", str(args.block)]
        rc = subprocess.run(cmd, env={**os.environ, **env}).returncode
        if rc:
            raise SystemExit(f"step {step}: exit status {rc}; no further step was started")
        with open(part) as f:
            res.update(json.load(f))
        os.remove(part)
    a, b, c = res["a_tree"], res["b_route"], res["c_path_load"]
    digests = {"a": a["digest"], "b": b["digest"], "c": c["digest"]}
    if len(set(digests.values())) != 1:
        raise SystemExit(f"legs a, b and c give different sums: {digests}")
    res["abc_sums_equal"] = True
    if a["info"]["tree"] == 0 or b["info"]["tree"] != 0:
        raise SystemExit(f"the tree tier switch did not take: a {a['info']}, b {b['info']}")
    spread = lambda r: r["device_ms"]["max"] - r["device_ms"]["min"]
    for other, name in ((b, "b"), (c, "c")):
        res[f"a_below_{name}_by_more_than_spreads"] = bool(
            other["device_ms"]["median"] - a["device_ms"]["median"] > spread(a) + spread(other))
        res[f"{name}_over_a_device"] = other["device_ms"]["median"] / a["device_ms"]["median"]
    if "a_counters" in res:
        i = res["a_counters"]["info"]
        res["commit_global_adds_per_claimed_entry"] = i["atomics"] / max(1, i["claimed"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c4")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sources", type=int, default=1024, help="rows of legs a, b and c")
    ap.add_argument("--block", type=int, default=2048, help="rows per call of leg e")
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(a child of the protocol)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--leg-e", action="store_true", help="also all rows with a weight matrix, in row blocks")
    ap.add_argument("--counters", action="store_true", help="also leg a with debug counters")
    ap.add_argument("--out", default=None, help="default: profiles/table_load_<config>shape.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", f"table_load_{args.config}shape.json")
    if args.step:
        res = STEPS[args.step](args)
        with open(args.out, "w") as f:
            json.dump(res, f)
        return
    run_steps(args)


if __name__ == "__main__":
    main()
